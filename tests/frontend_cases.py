"""The feature front end (fft.hip: trunet_stft_features, trunet_pcen, their `_fl` and ragged siblings, the lockstep
trunet_stream_features) through the C ABI against tests/frontend_ref.py: seeded inputs, launches, the comparison and the
report lines of tests/test_frontend_pin_gpu.py.  tests/test_frontend_ref_cpu.py feeds the same `judge_*` functions with
the restatement (and with its mutants) in place of kernel output.

Every family has  *_inputs(case) -> c,  *_gpu(c) -> got,  *_emul(c, mut) -> got (no GPU),  judge_*(c, got).

Launch hygiene (tests/bn_cases.py's `Sent`): every output is prefilled with NaN and has a sentinel region behind it in the
same allocation; every element of every output is compared, no bin is masked out.

What is compared (U = 2^-24; the counts are in tests/frontend_ref.py).  Per frame E_f = max_k |X_yard[k] - X_64[k]| over
both fp32 orders of the restatement (each transforms the PAIR, so E_f has the partner's leak), never the kernel:
  a. mag     |mag - mag64| <= d,  d = 4 E_f + 14 U (||frame||_2 + ||partner||_2)
  b. nm      against the float64 formula at the kernel's OWN fp32 mag, bit-read: the pointwise chain's counted roundings;
             exactly -1 at and below the floor, exactly +1 where the float64 value is above 1 by more than the roundings
  c. sin/cos |sin^2 + cos^2 - 1| <= 10 U where mag > 0, exactly (0, 1) where mag == 0, |mag (cos, sin) - X_64| <= d + 2 U mag64
  d. PCEN    on GIVEN magnitudes: convt_ref.close against the worse of the multiply-add and the fused yardstick
  e. lockstep  mag is not exposed: nm and PCEN (increasing in its own v, decreasing in earlier ones) inside the float64
             interval spanned by mag64 -+ d, widened by the roundings of b / d; the direction as in c with 2 d; pcen_M inside
             the same interval's smoother
  f. bits    `_fl` and ragged equal the dense entry point; a repeat launch and a launch with mag = NULL give the same bits;
             the ring after a hop is the exact shift; frames-last columns n >= N are zeros; channel 1 of C = 4 stays NaN
  silent     a frame whose 512 staged samples are exactly zero: mag == 0, nm == -1, (sin, cos) == (0, 1), PCEN 0 within d."""
import functools
import hashlib
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bn_cases as BC  # noqa: E402
import convt_cases as CC  # noqa: E402
import convt_ref as CR  # noqa: E402
import frontend_ref as R  # noqa: E402

U = R.U
NAN = BC.NAN
f64 = torch.float64
PARITY = "parity_frontend.txt"
Sent = BC.Sent
rejected = BC.rejected
NF, HOPF, BINS = R.NF, R.HOPF, R.BINS
PCEN_ARGS = (R.EPS, R.S, R.ALPHA, R.DELTA, R.RPOW)


class Judge(BC.Judge):
    """tests/bn_cases.py's collector (convt_ref.close and element-wise derived bounds), reporting to parity_frontend.txt"""

    def within(self, name, got, ref64, bnd):
        if tuple(got.shape) != tuple(ref64.shape):
            self.fails.append("%s %s: shape %s, expected %s" % (self.tag, name, tuple(got.shape), tuple(ref64.shape)))
            return
        super().within(name, got, ref64, bnd)

    def close(self, name, got, ref64, yard):
        if tuple(got.shape) != tuple(ref64.shape):
            self.fails.append("%s %s: shape %s, expected %s" % (self.tag, name, tuple(got.shape), tuple(ref64.shape)))
            return
        super().close(name, got, ref64, yard)

    def bits(self, name, got, want):
        self.exact(got.shape == want.shape and torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)),
                   "%s differs bit for bit" % name)

    def done(self):
        if not self.quiet:
            CC.report("%s: kernel error / e_y / bound  %s" % (self.tag, "  ".join(self.figs)), PARITY)
        assert not self.fails, "\n".join(self.fails)


def _gen(*key):
    return torch.Generator().manual_seed(int(hashlib.sha1(repr(key).encode()).hexdigest()[:8], 16))


def _rn(g, *s):
    return torch.randn(*s, generator=g, dtype=torch.float32)


def _lib():
    from tinyrecurrentunet_amd import _lib as Lb
    return Lb, Lb.lib()


def _tw():
    from tinyrecurrentunet_amd import _lib as Lb
    return Lb.twiddles(NF, torch.device("cuda"))


def _cpu(d):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


def same_bits(a, b, what):
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), "%s: %s differs on a repeat launch" % (what, k)


# ============================================================================================== STFT features
# L: 257 the smallest legal length, both reflections land on samples 0 and L - 1 (T = 3); 383 the longest tail inside one
# hop (T = 3); 384 even T (4); 640 a multiple of 128 (T = 6); 1153 several pairs (T = 10); 1025: odd T with several pairs
# (T = 9), where a lone last frame can be quiet next to a loud frame before it (what the zero partner protects)
FEAT_L = (257, 383, 384, 640, 1153, 1025)
FEAT_B = 3
# three different signals per case, so a wrong `b` stride shows
SIGSETS = {
    "noise": ("gauss0.1", "gauss0.1b", "gauss30"),          # amplitude 30: nm reaches +1
    "tonal": ("tone", "impulse", "dc"),                     # most bins near zero: the conditioning a strong-bin mask hides
    "quiet": ("gauss1e-9", "zeros", "fade"),                # every bin under the floor; exact zeros; a quiet lone last frame
    "silence": ("lead0.5", "tail0.5", "lead0.1"),           # exactly-zero frames on either side of a pair, next to loud ones
}
FEAT_CASES = [(L, C, sg) for L in FEAT_L for sg in SIGSETS for C in (3, 4)]
# frames-last edges: N = B T = 256 exactly (NP = 256 is full) and one column short
FL_EDGE_CASES = ((64, 384), (85, 257))
# ragged: different lengths, an odd-T utterance whose quiet last frame is followed by a loud utterance
RAGGED_CASES = (((257, "gauss0.1"), (1025, "fade"), (640, "lead0.5"), (383, "gauss30"), (384, "tail0.5"), (1153, "tone")),
                ((384, "zeros"), (257, "impulse"), (640, "tail0.5")))


def feat_id(case):
    return "L%d-C%d-%s" % case


def signal(kind, L, key):
    g = _gen("feat-signal", kind, L, key)
    T = R.nframes(L)
    n = torch.arange(L, dtype=f64)
    if kind.startswith("gauss"):
        return float(kind[5:].rstrip("b")) * _rn(g, L)
    if kind == "tone":
        return (0.5 * torch.cos(2.0 * torch.pi * 37.0 * n / NF + 0.3)).float()
    if kind == "impulse":
        x = torch.zeros(L)
        x[L // 2 + 3] = 0.8
        return x
    if kind == "dc":
        return torch.full((L,), 0.3)
    if kind == "zeros":
        return torch.zeros(L)
    last0 = (T - 1) * HOPF - NF // 2                      # first sample the last frame reads
    if kind == "fade":                                    # loud up to where the last frame begins, 1e-6 from there on
        cut = last0 if last0 > 0 else L // 2
        x = 0.5 * _rn(g, L)
        x[cut:] = 1e-6 * _rn(g, L - cut)
        return x
    amp = float(kind[4:])
    x = amp * _rn(g, L)
    if kind.startswith("lead"):                           # frame 0 reads samples 0 .. 256
        x[:NF // 2 + 1] = 0.0
    else:                                                 # tail: the last frame reads samples last0 .. L - 1
        x[(last0 if last0 > 0 else L - 100):] = 0.0
    return x


def _feat_refs(xs, C):
    """the float64 reference, both fp32 orders and the per-frame bound d of a list of utterances"""
    c = types.SimpleNamespace(xs=xs, C=C, lengths=[int(x.shape[0]) for x in xs])
    c.ref = R.features(xs, C)
    c.ya, c.yb = (R.features(xs, C, torch.float32, od) for od in ("dft", "fft"))
    Ef = torch.zeros(c.ref["re"].shape[0], dtype=f64)
    for y in (c.ya, c.yb):
        e = torch.sqrt((y["re"].double() - c.ref["re"]) ** 2 + (y["im"].double() - c.ref["im"]) ** 2).max(-1).values
        Ef = torch.maximum(Ef, e)
    c.Ef = Ef
    c.norms = c.ref["frames"].norm(dim=-1) + c.ref["partner"].norm(dim=-1)
    c.d = (CR.CLOSE_C * Ef + R.F_MAG * c.norms)[:, None]
    c.silent = (c.ref["frames"] == 0).all(-1)
    c.N = c.ref["re"].shape[0]
    return c


@functools.lru_cache(maxsize=None)
def feat_inputs(case):
    L, C, sg = case
    c = _feat_refs([signal(k, L, b) for b, k in enumerate(SIGSETS[sg])], C)
    c.case, c.tag, c.L, c.B, c.T = case, "FEATURES " + feat_id(case), L, FEAT_B, R.nframes(L)
    return c


@functools.lru_cache(maxsize=None)
def fl_edge_inputs(case):
    B, L = case
    g = _gen("fl-edge", case)
    c = _feat_refs([0.1 * _rn(g, L) for _ in range(B)], 4)
    c.case, c.tag, c.L, c.B, c.T = case, "FEATURES-FL-EDGE B%d-L%d" % case, L, B, R.nframes(L)
    return c


@functools.lru_cache(maxsize=None)
def ragged_inputs(i, C):
    spec = RAGGED_CASES[i]
    c = _feat_refs([signal(k, L, ("ragged", b)) for b, (L, k) in enumerate(spec)], C)
    c.case, c.tag, c.B = (i, C), "FEATURES-RAGGED %d-C%d" % (i, C), len(spec)
    c.off = R.ragged_offsets(c.lengths)
    return c


def _dense_launch(s, x, B, L, T, C, with_mag=True):
    Lb, lib = _lib()
    p = Lb.ptr
    feat = s.out(B * T, C, BINS)
    mag = s.out(B * T, BINS) if with_mag else None
    Lb.check(lib.trunet_stft_features(p(x), p(feat), p(mag), p(_tw()), B, L, T, C, Lb.stream()), "stft_features")
    return feat, mag


def _fl_launch(s, x, B, L, T, C, NP):
    Lb, lib = _lib()
    p = Lb.ptr
    xo, mag = s.out(C, BINS, NP), s.out(BINS, NP)
    Lb.check(lib.trunet_stft_features_fl(p(x), p(xo), p(mag), p(_tw()), B, L, T, C, NP, Lb.stream()), "stft_features_fl")
    return xo, mag


def feat_gpu(c, fl=(256, 512)):
    """dense (with mag, and again with mag = NULL) and frames-last at every NP of `fl` that holds N"""
    s = Sent()
    x = s.put(torch.stack(c.xs))
    o = {}
    o["feat"], o["mag"] = _dense_launch(s, x, c.B, c.L, c.T, c.C)
    o["feat_nomag"], _ = _dense_launch(s, x, c.B, c.L, c.T, c.C, with_mag=False)
    for NP in fl:
        if NP >= c.N:
            o["fl%d_x" % NP], o["fl%d_mag" % NP] = _fl_launch(s, x, c.B, c.L, c.T, c.C, NP)
    s.check(c.tag)
    return _cpu(o)


def ragged_gpu(c):
    """the ragged entry point on the packed batch, and the dense one on every utterance alone"""
    Lb, lib = _lib()
    p = Lb.ptr
    s = Sent()
    x = s.put(torch.cat(c.xs))
    so, fo, po = (t.cuda() for t in c.off)
    o = {"feat": s.out(c.N, c.C, BINS), "mag": s.out(c.N, BINS)}
    Lb.check(lib.trunet_stft_features_ragged(p(x), so.data_ptr(), fo.data_ptr(), po.data_ptr(), p(o["feat"]), p(o["mag"]),
                                             p(_tw()), c.B, int(c.off[0][-1]), int(c.off[1][-1]), int(c.off[2][-1]), c.C,
                                             Lb.stream()), "stft_features_ragged")
    df, dm = [], []
    for xb in c.xs:
        L = int(xb.shape[0])
        f, m = _dense_launch(s, s.put(xb[None]), 1, L, R.nframes(L), c.C)
        df.append(f)
        dm.append(m)
    s.check(c.tag)
    o["dense_feat"], o["dense_mag"] = torch.cat(df), torch.cat(dm)
    return _cpu(o)


def _feat_of(y):
    return {"feat": y["feat"].float(), "mag": y["mag"].float()}


def feat_emul(c, mut=None, order="fft", fl=(256, 512)):
    """the fp32 restatement (`order`) with `mut` in place of every launch of feat_gpu"""
    o = _feat_of(R.features(c.xs, c.C, torch.float32, order, mut))
    o["feat_nomag"] = o["feat"].clone()
    for NP in fl:
        if NP >= o["feat"].shape[0]:
            x = R.to_fl(o["feat"], NP)
            if c.C == 4:
                x[1] = NAN
            o["fl%d_x" % NP], o["fl%d_mag" % NP] = x, R.to_fl(o["mag"], NP)
    return o


def ragged_emul(c, mut=None, order="fft"):
    o = _feat_of(R.features(c.xs, c.C, torch.float32, order, None if mut == "ragged_pairs_across_utterances" else mut,
                            pair_across=mut == "ragged_pairs_across_utterances"))
    d = _feat_of(R.features(c.xs, c.C, torch.float32, order, None))
    o["dense_feat"], o["dense_mag"] = d["feat"], d["mag"]
    return o


def _judge_channels(j, c, feat, mag):
    """a - c and the silent frames, on a dense feat (N, C, 257) and mag (N, 257)"""
    C, ref = c.C, c.ref
    if tuple(feat.shape) != (c.N, C, BINS) or tuple(mag.shape) != (c.N, BINS):
        j.fails.append("%s: shapes %s %s, expected (%d, %d, 257)" % (j.tag, tuple(feat.shape), tuple(mag.shape), c.N, C))
        return
    nm, sn, cs = feat[:, 0], feat[:, C - 2], feat[:, C - 1]
    j.within("mag", mag, ref["mag"], c.d)
    raw, bnd = R.nm_raw64(mag)
    j.within("nm", nm, raw.clamp(-1.0, 1.0), bnd)
    j.exact((nm[mag <= R.f32(1e-7)] == -1).all() and (nm[raw < -1 - bnd] == -1).all(), "nm is not exactly -1 below the floor")
    j.exact((nm[raw > 1 + bnd] == 1).all(), "nm is not exactly +1 above 10^1.25")
    live = mag > 0
    unit = sn.double() ** 2 + cs.double() ** 2
    j.within("sin2+cos2", torch.where(live, unit, torch.ones((), dtype=f64)), torch.ones_like(unit), R.UNIT_BOUND)
    j.exact((sn[~live] == 0).all() and (cs[~live] == 1).all(), "(sin, cos) is not exactly (0, 1) where mag == 0")
    db = c.d + 2 * U * ref["mag"]
    j.within("mag*cos", mag.double() * cs.double(), ref["re"], db)
    j.within("mag*sin", mag.double() * sn.double(), ref["im"], db)
    if C == 4:
        j.exact(torch.isnan(feat[:, 1]).all(), "channel 1 of a C = 4 call was written")
    z = c.silent
    j.exact((mag[z] == 0).all() and (nm[z] == -1).all() and (sn[z] == 0).all() and (cs[z] == 1).all(),
            "an exactly silent frame is not (mag 0, nm -1, sin 0, cos 1): max |X| %.3e" % float(mag[z].abs().max() if z.any() else 0))


def judge_feat(c, got, quiet=False):
    j = Judge(c.tag, quiet)
    _judge_channels(j, c, got["feat"], got["mag"])
    j.bits("feat with mag = NULL", got["feat_nomag"], got["feat"])
    for k in sorted(got):
        if k.startswith("fl") and k.endswith("_x"):
            NP = int(k[2:-2])
            x, m = got[k], got["fl%d_mag" % NP]
            if tuple(x.shape) != (c.C, BINS, NP) or NP < got["feat"].shape[0]:
                j.fails.append("%s %s: shape %s" % (j.tag, k, tuple(x.shape)))
                continue
            N = got["feat"].shape[0]
            (xd, xt), (md, mt) = R.from_fl(x, N), R.from_fl(m, N)
            j.bits("_fl x (NP %d)" % NP, xd, got["feat"])
            j.bits("_fl mag (NP %d)" % NP, md, got["mag"])
            wr = [0, c.C - 2, c.C - 1]
            j.exact(BC.is_pos_zero(xt[wr]) and BC.is_pos_zero(mt), "_fl columns n >= N are not zeros (NP %d)" % NP)
            if c.C == 4:
                j.exact(torch.isnan(x[1]).all(), "_fl channel 1 of a C = 4 call was written")
    j.done()


def judge_ragged(c, got, quiet=False):
    j = Judge(c.tag, quiet)
    _judge_channels(j, c, got["feat"], got["mag"])
    j.bits("ragged feat against the dense entry point", got["feat"], got["dense_feat"])
    j.bits("ragged mag against the dense entry point", got["mag"], got["dense_mag"])
    j.done()


def silent_figures(c, feat, mag):
    """(number of exactly silent frames, max |X| over them, are their four channels exact)"""
    z = c.silent
    if not bool(z.any()):
        return 0, 0.0, True
    nm, sn, cs = feat[:, 0][z], feat[:, c.C - 2][z], feat[:, c.C - 1][z]
    ok = bool((mag[z] == 0).all() and (nm == -1).all() and (sn == 0).all() and (cs == 1).all())
    return int(z.sum()), float(mag[z].abs().max()), ok


# ============================================================================================== PCEN on given magnitudes
# T around the 256-frame chunk of pcen_scan_kernel and the 128-frame chunk of pcen_scan_fl_kernel
PCEN_T = (1, 2, 127, 128, 129, 255, 256, 257, 513)
PCEN_B = 2
PCEN_SETS = (("generic", "zeros_burst"), ("burst_zeros", "spike"), ("zeros", "generic"))
PCEN_CASES = [(T, (1, 4)[(iT + iS) % 2], iS) for iT, T in enumerate(PCEN_T) for iS in range(len(PCEN_SETS))]
PCEN_RAGGED_T = (3, 256, 2)             # the restart lands inside a chunk (frame 3) and on a chunk's edge (frame 259)


def pcen_id(case):
    return "T%d-stride%dx257-%s" % (case[0], case[1], "+".join(PCEN_SETS[case[2]]))


def magnitudes(kind, T, key):
    g = _gen("pcen-mag", kind, T, key)
    v = (3.0 * _rn(g, T, BINS)).abs() * torch.rand(1, BINS, generator=g)
    h = (T + 1) // 2
    if kind == "zeros_burst":
        v[:h] = 0.0
    elif kind == "burst_zeros":
        v[h:] = 0.0
    elif kind == "zeros":
        v[:] = 0.0
    elif kind == "spike":
        v[T // 3, ::7] = 1e4
    return v


def _pcen_refs(mags):
    c = types.SimpleNamespace(mags=mags)
    c.ref = R.pcen(mags)
    c.yard = R.yardstick(c.ref, *(R.pcen(mags, torch.float32, od) for od in ("dft", "fft")))
    c.N = c.ref.shape[0]
    return c


@functools.lru_cache(maxsize=None)
def pcen_inputs(case):
    T, nch, iS = case
    c = _pcen_refs([magnitudes(k, T, b) for b, k in enumerate(PCEN_SETS[iS])])
    c.case, c.tag, c.T, c.B, c.nch = case, "PCEN " + pcen_id(case), T, PCEN_B, nch
    c.zero = torch.cat([torch.full((T,), k == "zeros") for k in PCEN_SETS[iS]])
    return c


@functools.lru_cache(maxsize=None)
def pcen_ragged_inputs():
    kinds = ("generic", "zeros_burst", "spike")
    c = _pcen_refs([magnitudes(k, T, ("ragged", b)) for b, (T, k) in enumerate(zip(PCEN_RAGGED_T, kinds))])
    c.case, c.tag, c.B, c.nch = "ragged", "PCEN-RAGGED T%d+%d+%d" % PCEN_RAGGED_T, len(kinds), 4
    fo = [0]
    for T in PCEN_RAGGED_T:
        fo.append(fo[-1] + T)
    c.fo = torch.tensor(fo, dtype=torch.int64)
    c.zero = torch.zeros(c.N, dtype=torch.bool)
    return c


def _pcen_dense_launch(s, mag, B, T, nch):
    """out = channel 1 of an (B T, nch, 257) image (nch = 1: the image is the output)"""
    Lb, lib = _lib()
    img = s.out(B * T, nch, BINS)
    ch = 1 if nch > 1 else 0
    out_ptr = img.data_ptr() + 4 * ch * BINS
    Lb.check(lib.trunet_pcen(Lb.ptr(mag), out_ptr, B, T, nch * BINS, *PCEN_ARGS, Lb.stream()), "pcen")
    return img


def pcen_gpu(c):
    Lb, lib = _lib()
    s = Sent()
    mag = s.put(torch.cat(c.mags))
    o = {"img": _pcen_dense_launch(s, mag, c.B, c.T, c.nch)}
    NP = -(-c.N // 256) * 256
    mfl = R.to_fl(torch.cat(c.mags), NP)
    mfl[:, c.N:] = NAN                                    # what lies in the columns n >= N must not matter
    o["fl"] = s.out(BINS, NP)
    Lb.check(lib.trunet_pcen_fl(Lb.ptr(s.put(mfl)), Lb.ptr(o["fl"]), c.B, c.T, NP, *PCEN_ARGS, Lb.stream()), "pcen_fl")
    s.check(c.tag)
    return _cpu(o)


def pcen_ragged_gpu(c):
    Lb, lib = _lib()
    s = Sent()
    mag = s.put(torch.cat(c.mags))
    fo = c.fo.cuda()
    o = {"img": s.out(c.N, c.nch, BINS)}
    Lb.check(lib.trunet_pcen_ragged(Lb.ptr(mag), o["img"].data_ptr() + 4 * BINS, fo.data_ptr(), c.B, c.N, c.nch * BINS,
                                    *PCEN_ARGS, Lb.stream()), "pcen_ragged")
    o["dense_img"] = torch.cat([_pcen_dense_launch(s, s.put(m), 1, m.shape[0], c.nch) for m in c.mags])
    s.check(c.tag)
    return _cpu(o)


def _img(out, nch):
    img = torch.full((out.shape[0], nch, BINS), NAN)
    img[:, 1 if nch > 1 else 0] = out
    return img


def pcen_emul(c, mut=None, order="fft"):
    out = R.pcen(c.mags, torch.float32, order, mut)
    o = {"img": _img(out, c.nch)}
    if c.case == "ragged":
        o["dense_img"] = _img(torch.cat([R.pcen([m], torch.float32, order, mut) for m in c.mags]), c.nch)
    else:
        o["fl"] = R.to_fl(out, -(-c.N // 256) * 256)
    return o


def judge_pcen(c, got, quiet=False):
    j = Judge(c.tag, quiet)
    img = got["img"]
    ch = 1 if c.nch > 1 else 0
    out = img[:, ch]
    j.close("pcen", out, c.ref, c.yard)
    j.exact(BC.is_pos_zero(out[c.zero]) if bool(c.zero.any()) else True, "an all-zero utterance does not give exact zeros")
    rest = [k for k in range(c.nch) if k != ch]
    j.exact(torch.isnan(img[:, rest]).all(), "a channel next to the output was written")
    if "fl" in got:
        d, t = R.from_fl(got["fl"], c.N)
        j.bits("_fl against the dense entry point", d, out)
        j.exact(BC.is_pos_zero(t), "_fl columns n >= N are not zeros")
    if "dense_img" in got:
        j.bits("ragged against the dense entry point", img, got["dense_img"])
    j.done()


# ============================================================================================== lockstep stream
STREAM_S = (1, 2, 3)                    # odd S: a lone stream in its block
STREAM_HOPS = 5
STREAM_REGIMES = ("loud", "mute0", "mute1")         # a silent stream beside a loud one, on either side of the pair
STREAM_CASES = [(S, C, rg) for S in STREAM_S for C in (4, 3) for rg in STREAM_REGIMES if not (rg == "mute1" and S == 1)
                and not (C == 3 and rg != "loud")]
STREAM_AMP = (0.1, 0.5, 0.02)


def stream_id(case):
    return "S%d-C%d-%s" % case


@functools.lru_cache(maxsize=None)
def stream_inputs(case):
    S, C, rg = case
    g = _gen("stream", case)
    amp = torch.tensor(STREAM_AMP[:S])
    if rg != "loud":
        amp[int(rg[-1])] = 0.0
        amp[amp > 0] = 0.5
    c = types.SimpleNamespace(case=case, tag="STREAM " + stream_id(case), S=S, C=C)
    c.ring0 = amp[:, None] * _rn(g, S, NF)
    c.chunks = amp[None, :, None] * _rn(g, STREAM_HOPS, S, HOPF)
    c.ref = R.stream(c.ring0, c.chunks, C)
    ya, yb = (R.stream(c.ring0, c.chunks, C, torch.float32, od) for od in ("dft", "fft"))
    Ef = torch.zeros(c.ref["re"].shape[:2], dtype=f64)
    for y in (ya, yb):
        e = torch.sqrt((y["re"].double() - c.ref["re"]) ** 2 + (y["im"].double() - c.ref["im"]) ** 2).max(-1).values
        Ef = torch.maximum(Ef, e)
    c.d = (CR.CLOSE_C * Ef + R.F_MAG * (c.ref["frames"].norm(dim=-1) + c.ref["partner"].norm(dim=-1)))[..., None]
    c.silent = (c.ref["frames"] == 0).all(-1)                          # (H + 1, S)
    v = c.ref["mag"]
    if C == 4:
        # d: the yardstick's PCEN on the reference's own magnitudes, against float64 of the same
        vs = [v[:, i].float() for i in range(S)]
        r64 = torch.stack([R.pcen([m]) for m in vs], 1)
        y32 = torch.stack([R.yardstick(R.pcen([m]), *(R.pcen([m], torch.float32, od) for od in ("dft", "fft"))) for m in vs], 1)
        c.w = CR.bound(r64, y32)[1]
        M64 = torch.stack([R.smooth(m) for m in vs], 1)
        M32 = torch.stack([R.yardstick(R.smooth(m), *(R.smooth(m, None, torch.float32, od) for od in ("dft", "fft"))) for m in vs], 1)
        c.wM = CR.bound(M64, M32)[1]
        up, dn = v + c.d, (v - c.d).clamp_min(0.0)
        c.p_hi, c.p_lo, c.M_hi, c.M_lo = [], [], None, None
        hi, lo = [], []
        for h in range(v.shape[0]):
            vh = torch.cat([dn[:h], up[h:h + 1]])                      # own v up, earlier ones down
            vl = torch.cat([up[:h], dn[h:h + 1]])
            Mh = torch.stack([R.smooth(vh[:, i]) for i in range(S)], 1)
            Ml = torch.stack([R.smooth(vl[:, i]) for i in range(S)], 1)
            hi.append(R.pcen_value(vh[h], Mh[h]))
            lo.append(R.pcen_value(vl[h], Ml[h]))
        c.p_hi, c.p_lo = torch.stack(hi), torch.stack(lo)
        c.M_hi = torch.stack([R.smooth(up[:, i]) for i in range(S)], 1)[-1]
        c.M_lo = torch.stack([R.smooth(dn[:, i]) for i in range(S)], 1)[-1]
    return c


def stream_gpu(c):
    Lb, lib = _lib()
    p = Lb.ptr
    s = Sent()
    ring, M = s.put(c.ring0), s.out(c.S, BINS)
    feats, rings = [], []
    for h in range(STREAM_HOPS + 1):
        feat = s.out(c.S, c.C, BINS)
        chunk = s.put(c.chunks[h - 1]) if h > 0 else None
        Lb.check(lib.trunet_stream_features(p(ring), p(chunk), p(M), p(feat), p(_tw()), c.S, c.C, 1 if h == 0 else 0,
                                            *PCEN_ARGS, Lb.stream()), "stream_features")
        torch.cuda.synchronize()
        feats.append(feat.clone())
        rings.append(ring.clone())
    s.check(c.tag)
    return _cpu({"feat": torch.stack(feats), "ring": torch.stack(rings), "pcen_M": M})


def stream_emul(c, mut=None, order="fft"):
    y = R.stream(c.ring0, c.chunks, c.C, torch.float32, order, mut)
    M = y["pcen_M"].float() if c.C == 4 else torch.full((c.S, BINS), NAN)
    return {"feat": y["feat"].float(), "ring": y["ring"].float(), "pcen_M": M}


def _mid(lo, hi):
    return 0.5 * (lo + hi), 0.5 * (hi - lo)


def judge_stream(c, got, quiet=False):
    j = Judge(c.tag, quiet)
    C, ref = c.C, c.ref
    feat = got["feat"]
    j.bits("ring", got["ring"], ref["ring"].float())
    if tuple(feat.shape) != tuple(ref["feat"].shape):
        j.fails.append("%s: feat shape %s" % (j.tag, tuple(feat.shape)))
        j.done()
    nm, sn, cs = feat[:, :, 0], feat[:, :, C - 2], feat[:, :, C - 1]
    v = ref["mag"]
    (r_hi, b_hi), (r_lo, b_lo) = R.nm_raw64((v + c.d).float()), R.nm_raw64((v - c.d).clamp_min(0.0).float())
    mid, half = _mid(r_lo.clamp(-1, 1) - b_lo, r_hi.clamp(-1, 1) + b_hi)
    j.within("nm", nm, mid, half)
    unit = sn.double() ** 2 + cs.double() ** 2
    j.within("sin2+cos2", unit, torch.ones_like(unit), R.UNIT_BOUND)
    db = 2 * c.d + 2 * U * v
    j.within("mag64*cos", v * cs.double(), ref["re"], db)
    j.within("mag64*sin", v * sn.double(), ref["im"], db)
    z = c.silent
    j.exact((nm[z] == -1).all() and (sn[z] == 0).all() and (cs[z] == 1).all(),
            "an exactly silent stream is not (nm -1, sin 0, cos 1)")
    if C == 4:
        mid, half = _mid(c.p_lo - c.w, c.p_hi + c.w)
        # an exactly silent stream: the interval would be as wide as the design allows a NEARLY silent frame; its value is 0
        zz = z[..., None].expand_as(mid)
        mid, half = torch.where(zz, torch.zeros_like(mid), mid), torch.where(zz, torch.full_like(half, c.w), half)
        j.within("pcen", feat[:, :, 1], mid, half)
        mid, half = _mid(c.M_lo - c.wM, c.M_hi + c.wM)
        j.within("pcen_M", got["pcen_M"], mid, half)
        if bool(z.any()):
            j.within("pcen@silent", feat[:, :, 1][z], torch.zeros(int(z.sum()), BINS, dtype=f64),
                     CR.CLOSE_F * float(ref["feat"][:, :, 1].abs().max()))
    else:
        j.exact(torch.isnan(got["pcen_M"]).all(), "pcen_M of a C = 3 call was written")
    j.done()


def interval_condition(c):
    """(e) is a statement only where the interval is narrower than the values it holds apart: the largest half-width of
    the PCEN interval of a stream that is not silent, relative to the largest PCEN value of the case"""
    if c.C != 4:
        return 0.0
    half = 0.5 * (c.p_hi - c.p_lo)[~c.silent]
    return float(half.max()) / float(c.ref["feat"][:, :, 1].abs().max()) if half.numel() else 0.0


# ============================================================================================== exactly silent frames
# the cases above that hold frames whose 512 staged samples are exactly zero next to loud ones (amplitudes 0.1 and 0.5),
# through every entry point that pairs two frames, with PCEN behind the kernel's own magnitudes
SILENT_L = (384, 640, 1025, 1153)


def silent_gpu(L):
    """{entry: (feat (N, 4, 257) with PCEN in channel 1, mag (N, 257))} for dense, _fl and ragged on the `silence` signals"""
    Lb, lib = _lib()
    p = Lb.ptr
    c = feat_inputs((L, 4, "silence"))
    s = Sent()
    x = s.put(torch.stack(c.xs))
    o = {}
    feat, mag = _dense_launch(s, x, c.B, c.L, c.T, 4)
    Lb.check(lib.trunet_pcen(p(mag), feat.data_ptr() + 4 * BINS, c.B, c.T, 4 * BINS, *PCEN_ARGS, Lb.stream()), "pcen")
    o["dense"] = (feat, mag)
    NP = 256
    xo, mfl = _fl_launch(s, x, c.B, c.L, c.T, 4, NP)
    Lb.check(lib.trunet_pcen_fl(p(mfl), xo.data_ptr() + 4 * BINS * NP, c.B, c.T, NP, *PCEN_ARGS, Lb.stream()), "pcen_fl")
    so, fo, po = (t.cuda() for t in R.ragged_offsets(c.lengths))
    rf, rm = s.out(c.N, 4, BINS), s.out(c.N, BINS)
    Lb.check(lib.trunet_stft_features_ragged(p(s.put(torch.cat(c.xs))), so.data_ptr(), fo.data_ptr(), po.data_ptr(), p(rf), p(rm),
                                             p(_tw()), c.B, int(so[-1]), int(fo[-1]), int(po[-1]), 4, Lb.stream()), "ragged")
    Lb.check(lib.trunet_pcen_ragged(p(rm), rf.data_ptr() + 4 * BINS, fo.data_ptr(), c.B, c.N, 4 * BINS, *PCEN_ARGS,
                                    Lb.stream()), "pcen_ragged")
    o["ragged"] = (rf, rm)
    s.check(c.tag)
    torch.cuda.synchronize()
    o["fl"] = (R.from_fl(xo.cpu(), c.N)[0], R.from_fl(mfl.cpu(), c.N)[0])
    return {k: (a.cpu(), b.cpu()) for k, (a, b) in o.items()}


def silent_emul(L, mut=None, order="fft"):
    c = feat_inputs((L, 4, "silence"))
    y = R.features(c.xs, 4, torch.float32, order, mut)
    feat, mag = y["feat"].float(), y["mag"].float()
    T = c.T
    feat[:, 1] = R.pcen([mag[b * T:(b + 1) * T] for b in range(c.B)], torch.float32, order, mut)
    return {k: (feat, mag) for k in ("dense", "fl", "ragged")}


def judge_silent(L, got, quiet=False):
    """every exactly silent frame: mag == 0, nm == -1, (sin, cos) == (0, 1), PCEN equal to the float64 value at v = 0 (0,
    whatever the smoother holds) within d's floor 8 U max|PCEN64|.  The report line has the frames, max |X| and max |PCEN| over
    them per amplitude."""
    c = feat_inputs((L, 4, "silence"))
    j = Judge("SILENT L%d" % L, quiet)
    T, z = c.T, c.silent
    p64 = R.pcen([c.ref["mag"][b * T:(b + 1) * T].float() for b in range(c.B)])
    floor = CR.CLOSE_F * float(p64.abs().max())
    for entry, (feat, mag) in sorted(got.items()):
        n, mx, ok = silent_figures(c, feat, mag)
        fig = "%s frames %d" % (entry, n)
        for b, kind in enumerate(SIGSETS["silence"]):
            zb = torch.zeros_like(z)
            zb[b * T:(b + 1) * T] = z[b * T:(b + 1) * T]
            if bool(zb.any()):
                fig += " %s max|X| %.2e max|pcen| %.2e" % (kind, float(mag[zb].abs().max()), float(feat[:, 1][zb].abs().max()))
        j.figs.append(fig)
        j.exact(ok, "%s: an exactly silent frame is not (mag 0, nm -1, sin 0, cos 1): max |X| %.3e" % (entry, mx))
        if n:
            j.within("%s pcen@silent" % entry, feat[:, 1][z], torch.zeros(n, BINS, dtype=f64), floor)
    j.done()
    return n
