"""The band above 8 kHz around a 16 kHz enhancement (tinyrecurrentunet_amd/highband.py) without a GPU:
the high-pass's response, the frame gains and the split / rejoin arithmetic of the float64 restatement
(tests/highband_ref.py), the tone that "drop" loses and "keep" returns, the integer gain index, the entry points' and the
host's refusals and the command line."""
import os
import re

import numpy as np
import pytest

import highband_ref as HR
import resample_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every rate above 16 kHz that resample.py names
RATES = (22050, 24000, 32000, 44100, 48000, 88200, 96000)


def test_highpass_response_and_the_package_taps():
    """at most -80 dB up to 3.25 kHz, within +-0.01 dB from 4.75 kHz (measured: -86.7 dB and +0.0004 dB)"""
    from tinyrecurrentunet_amd import highband as HB
    hp = HR.highpass()
    assert hp.shape == (63,) and hp.dtype == np.float64 and np.array_equal(hp, hp[::-1])
    assert np.array_equal(hp, HB.highpass())
    assert abs(np.sum(hp)) < 1e-12                                          # no gain at 0 Hz
    n = 1 << 16
    H = 20 * np.log10(np.maximum(np.abs(np.fft.rfft(hp, n)), 1e-300))
    f = np.arange(H.shape[0]) * 16000.0 / n
    print("hp: %.2f dB up to 3.25 kHz, %+.5f .. %+.5f dB from 4.75 kHz" % (H[f <= 3250].max(), H[f >= 4750].min(),
                                                                          H[f >= 4750].max()))
    assert H[f <= 3250].max() <= -80.0
    assert np.abs(H[f >= 4750]).max() <= 0.01


def test_header_constants_match_the_module():
    from tinyrecurrentunet_amd import highband as HB
    hdr = open(os.path.join(ROOT, "include", "trunet_hip.h")).read()
    val = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))
    assert (val("TRUNET_HB_TAPS"), val("TRUNET_HB_KEEP"), val("TRUNET_HB_FOLLOW")) == (HB.TAPS, HB.KEEP, HB.FOLLOW)
    assert (val("TRUNET_HB_RUN"), val("TRUNET_HB_JOIN_TILE")) == (HB.RUN, HB.JOIN_TILE)
    assert HB.TAPS == HR.TAPS == 2 * HB.HALF + 1 and HB.HOP == HR.HOP == 128
    assert HB.MODES == ("drop", "keep", "follow")
    # the fp32 clamp value: -30 dB by default, never zero
    assert abs(HB.floor_gain(-30.0) - HR.floor_gain(-30.0)) <= 2.0 ** -24 * HR.floor_gain(-30.0)
    assert HB.floor_gain(-30.0) == float(np.float32(HB.floor_gain(-30.0))) and HB.floor_gain(0) == 1.0
    assert HB.floor_gain(-5000.0) > 0.0


@pytest.mark.parametrize("L16", [257, 1000, 4096])
def test_gains_of_a_scaled_signal(L16):
    g = np.random.default_rng(L16)
    lo = g.standard_normal(L16)
    T = 1 + L16 // 128
    g_min = HR.floor_gain(-30.0)
    for c in (0.25, 1.0):
        v, _ = HR.gains(lo, c * lo)
        assert v.shape == (T,) and np.max(np.abs(v - c)) < 1e-8
    for c in (0.0, 0.01):
        assert np.array_equal(HR.gains(lo, c * lo)[0], np.full(T, g_min))
    assert np.array_equal(HR.gains(lo, 2.0 * lo)[0], np.ones(T))               # an enhancement that amplifies is capped
    assert np.array_equal(HR.gains(np.zeros(L16), np.zeros(L16))[0], np.ones(T))   # silence
    assert np.max(np.abs(HR.gains(lo, 0.01 * lo, floor_db=-60.0)[0] - 0.01)) < 1e-8
    # a frame's gain is local: changing y16 from sample 128 * 6 + 31 on leaves the frames up to t = 3 alone
    if L16 >= 1000:
        y = 0.5 * lo
        y2 = y.copy()
        y2[128 * 6 + 31:] = 0.0
        assert np.array_equal(HR.gains(lo, y)[0][:4], HR.gains(lo, y2)[0][:4])
        assert HR.gains(lo, y2)[0][5] < 0.5 - 1e-3


@pytest.mark.parametrize("fs", [48000, 44100, 32000])
def test_rejoin_restatement_is_exact_for_a_linear_enhancement(fs):
    g = np.random.default_rng(fs)
    x = g.standard_normal(3001)
    lo = HR.down(x, fs)
    assert np.max(np.abs(HR.rejoin(x, lo, lo, fs, "keep") - x)) < 1e-12
    assert np.max(np.abs(HR.rejoin(x, lo, 0.25 * lo, fs, "follow") - 0.25 * x)) < 1e-9      # g_min < 0.25: linear
    assert np.max(np.abs(HR.rejoin(x, lo, lo, fs, "follow") - x)) < 1e-9
    assert np.array_equal(HR.rejoin(x, lo, 0.25 * lo, fs, "drop"), HR.up(0.25 * lo, fs, x.shape[0]))


def _amplitude(v, f0, fs):
    """amplitude of the sine at f0 by projection over the middle half"""
    n = np.arange(v.shape[0])
    m = slice(v.shape[0] // 4, 3 * v.shape[0] // 4)
    return 2.0 * np.abs(np.sum(v[m] * np.exp(-2j * np.pi * f0 * n[m] / fs))) / (m.stop - m.start)


@pytest.mark.parametrize("fs,f0", [(48000, 12000), (44100, 12000), (96000, 12000), (32000, 11000)])
def test_tone_above_the_band_is_lost_by_drop_and_returned_by_keep(fs, f0):
    """one second of noise below 3 kHz plus a sine of amplitude 0.1 above 8 kHz, a stand-in enhancement y16 = lo / 2:
    below 1e-4 in U(y16) alone, within 1e-3 relative of 0.1 with "keep" (measured: at most 5e-6 and 3.4e-5)"""
    g = np.random.default_rng(f0 + fs)
    spec = np.fft.rfft(g.standard_normal(fs))
    spec[np.arange(spec.shape[0]) > 3000] = 0.0                              # bin k is k Hz: one second
    noise = np.fft.irfft(spec, fs)
    x = 0.1 * noise / np.max(np.abs(noise)) + 0.1 * np.sin(2 * np.pi * f0 * np.arange(fs) / fs + 0.3)
    lo = HR.down(x, fs)
    y16 = 0.5 * lo
    drop = HR.rejoin(x, lo, y16, fs, "drop")
    keep = HR.rejoin(x, lo, y16, fs, "keep")
    a_drop, a_keep = _amplitude(drop, f0, fs), _amplitude(keep, f0, fs)
    print("%d Hz in %d Hz: drop %.3e, keep off by %.3e relative" % (f0, fs, a_drop, abs(a_keep - 0.1) / 0.1))
    assert abs(_amplitude(x, f0, fs) - 0.1) < 1e-4 * 0.1                        # the measurement itself
    assert a_drop < 1e-4
    assert abs(a_keep - 0.1) <= 1e-3 * 0.1


@pytest.mark.parametrize("fs", RATES)
def test_gain_index_stays_inside_the_frames(fs):
    """t0 = n pd // (128 qd) <= T - 1 for every sample of every length that resamples to L16, and the 32-bit arithmetic of
    the kernel (one 64-bit division per tile of 4096 samples, c = c_tile + i pd per sample) is the int64 arithmetic"""
    from tinyrecurrentunet_amd import resample as R
    pd, qd = R.ratio(fs, 16000)
    assert (pd, qd) == RR.ratio(fs, 16000) and pd < qd
    D = 128 * qd
    for L16 in (257, 383, 384, 385):
        T = HR.n_frames(L16)
        lens = [L for L in range((L16 - 1) * qd // pd, L16 * qd // pd + 2) if R.out_length(L, pd, qd) == L16]
        assert lens
        for L in (lens[0], lens[-1]):
            t0, al = HR.gain_index(np.arange(L, dtype=np.int64), pd, qd)
            assert t0.max() <= T - 1 and al.min() >= 0.0 and al.max() < 1.0
    assert D - 1 + 4095 * pd < 2 ** 32
    n = np.array([0, 1, 4095, 4096, 4097, 2 ** 31 - 2], dtype=np.int64)
    tile = n // 4096 * 4096
    tt, ct = tile * pd // D, tile * pd % D
    c = ct + (n - tile) * pd
    t0, al = HR.gain_index(n, pd, qd)
    assert np.array_equal(tt + c // D, t0) and np.array_equal((c % D) / D, al)


def test_entry_points_refuse_before_they_launch():
    """nothing is launched, so dummy non-null pointers are safe"""
    from tinyrecurrentunet_amd import _lib
    lib = _lib.lib()
    EINVAL = _lib.TRUNET_EINVAL
    P = [0x1000 * (i + 1) for i in range(8)]
    ok = dict(B=2, nS=1000, nT=9, gmin=0.03)

    def gains(ptrs=P[:7], **kw):
        a = dict(ok, **kw)
        return lib.trunet_highband_gains(*ptrs, a["B"], a["nS"], a["nT"], a["gmin"], None)

    for k in range(7):
        assert gains(P[:k] + [None] + P[k + 1:7]) == EINVAL                 # every pointer is needed
    assert gains(B=0) == EINVAL
    assert gains(nS=-1) == EINVAL and gains(nS=2 ** 31) == EINVAL
    assert gains(nT=7) == EINVAL                                            # fewer frames than 1000 samples + 2 utterances have
    assert gains(nT=10) == EINVAL                                           # ... or more
    assert gains(gmin=0.0) == EINVAL and gains(gmin=1.5) == EINVAL and gains(gmin=float("nan")) == EINVAL

    okj = dict(B=2, nF=3000, nU=3010, nT=9, pd=1, qd=3, mode=2)

    def join(ptrs=P, **kw):
        a = dict(okj, **kw)
        return lib.trunet_highband_join(*ptrs, a["B"], a["nF"], a["nU"], a["nT"], a["pd"], a["qd"], a["mode"], None)

    for k in range(8):
        assert join(P[:k] + [None] + P[k + 1:]) == EINVAL
    keep = P[:3] + [None] + P[4:7] + [None]                                 # "keep" needs neither g nor the frame table
    assert join(keep, mode=1, nF=0, nU=0) == _lib.TRUNET_OK                 # nothing to do: no launch either
    assert join(keep, mode=2, nF=0, nU=0) == EINVAL
    assert join(B=0) == EINVAL and join(nF=-1) == EINVAL and join(nU=2999) == EINVAL and join(nU=2 ** 31) == EINVAL
    assert join(mode=0) == EINVAL and join(mode=3) == EINVAL
    assert join(pd=0) == EINVAL and join(pd=3) == EINVAL and join(pd=4) == EINVAL and join(qd=641) == EINVAL
    assert join(nT=1) == EINVAL and join(nT=26) == EINVAL


def test_enhance_and_rejoin_refuse_on_the_host():
    """a mode outside the three and a floor outside (-inf, 0] raise before anything reaches the device (or the network)"""
    from tinyrecurrentunet_amd import highband as HB
    from tinyrecurrentunet_amd.enhance import enhance
    for fs in (48000, 16000):
        with pytest.raises(ValueError, match="highband must be one of"):
            enhance(None, [], fs=fs, highband="restore")
        for bad in (0.5, float("nan"), float("-inf"), float("inf"), "low", None, True):
            with pytest.raises(ValueError, match="highband_floor_db"):
                enhance(None, [], fs=fs, highband="follow", highband_floor_db=bad)
    assert HB.check_args("keep", 0) == ("keep", 0.0) and HB.check_args("drop", np.float32(-12.5)) == ("drop", -12.5)
    for fs in (16000, 8000):
        with pytest.raises(ValueError, match="above 16000 Hz"):
            HB.rejoin([], [], [], fs)
    with pytest.raises(ValueError):
        HB.rejoin([], [], [], 16001)                                        # no ratio within 640
    with pytest.raises(ValueError, match="highband must be one of"):
        HB.rejoin([], [], [], 48000, mode="all")
    assert HB.rejoin([], [], [], 48000) == [] and HB.gains([], []) == []
    import torch
    with pytest.raises(ValueError, match="1-D tensor"):
        HB.rejoin([torch.zeros(2, 3)], [], [], 48000)
    with pytest.raises(_lib_error(), match="MI355X only"):
        HB.rejoin([torch.zeros(900)], [torch.zeros(300)], [torch.zeros(300)], 48000)


def _lib_error():
    from tinyrecurrentunet_amd import _lib
    return _lib.TrunetHipError


def test_command_line_takes_highband_with_resample_only(capsys):
    """the parser, in this process: every case ends in argparse's exit before a file or the device is touched"""
    from tinyrecurrentunet_amd.enhance import main

    def run(*argv):
        with pytest.raises(SystemExit) as e:
            main(list(argv))
        got = capsys.readouterr()
        return e.value.code, " ".join((got.out + got.err).split())

    code, text = run("--help")
    assert code == 0 and "--highband {drop,keep,follow}" in text and "--highband-floor-db" in text
    base = ("--checkpoint", "none.pkl", "--input-size", "4", "--in", "nowhere", "--out", "nowhere")
    code, text = run(*base, "--highband", "follow")
    assert code == 2 and "go with --resample" in text
    code, text = run(*base, "--resample", "--highband", "louder")
    assert code == 2 and "invalid choice" in text
    code, text = run(*base, "--resample", "--highband", "follow", "--highband-floor-db", "3")
    assert code == 2 and "highband_floor_db" in text
