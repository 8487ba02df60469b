"""The rational resampler (tinyrecurrentunet_amd/resample.py) without a GPU: the float64 restatement
against scipy, the filter's response, the ratio arithmetic, the phase-major tap table and the tile layout, the entry
point's refusals and every host-side refusal of resample / enhance(fs=...) / the dataset, and the command line's help."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import resample_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = [(1, 3), (3, 1), (160, 441), (441, 160), (640, 441), (2, 1)]
# every rate the module names, to and from 16 kHz
RATES = (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)


@pytest.mark.parametrize("pq", RATIOS)
def test_restatement_matches_scipy(pq):
    from scipy.signal import resample_poly
    p, q = pq
    h, half = RR.design(p, q)
    g = np.random.default_rng(p * 1000 + q)
    for n in (1, 2, 1000, 3001):
        x = g.standard_normal(n)
        y, _ = RR.resample(x, p, q)
        ref = resample_poly(x, p, q, window=h)
        assert y.shape == ref.shape == (-(-n * p // q),)
        assert np.max(np.abs(y - ref)) < 1e-12, (pq, n)


@pytest.mark.parametrize("pq", RATIOS + [(1, 6)])
def test_filter_response(pq):
    """pass band within +0.01 / -0.6 dB up to 0.85 Nyquist of the lower rate, at most -60 dB from 1.1 Nyquist upwards"""
    from tinyrecurrentunet_amd import resample as R
    p, q = pq
    h, half = R.design(p, q)
    hr, halfr = RR.design(p, q)
    assert half == halfr == 16 * max(p, q) and h.shape == (2 * half + 1,) and h.dtype == np.float64
    assert np.array_equal(h, hr)
    assert abs(np.sum(h) - 1.0) < 1e-12
    assert np.array_equal(h, h[::-1])
    n = 1 << 20
    H = 20 * np.log10(np.maximum(np.abs(np.fft.rfft(h, n)), 1e-300))
    f = np.arange(H.shape[0]) / n                    # cycles per sample at the rate the taps live at
    nyq = 0.5 / max(p, q)
    assert H[f <= 0.85 * nyq].min() >= -0.6 and H[f <= 0.85 * nyq].max() <= 0.01
    assert H[f >= 1.1 * nyq].max() <= -60.0


def test_ratio_reduces_and_refuses():
    from tinyrecurrentunet_amd import resample as R
    assert R.MAX_RATIO == 640
    assert R.ratio(48000, 16000) == (1, 3)
    assert R.ratio(44100, 16000) == (160, 441)
    assert R.ratio(11025, 16000) == (640, 441)
    assert R.ratio(16000, 16000) == (1, 1)
    for fs in RATES:
        p, q = R.ratio(fs, 16000)
        assert R.ratio(16000, fs) == (q, p) and math.gcd(p, q) == 1 and p * fs == q * 16000
        assert (p, q) == RR.ratio(fs, 16000)
    for bad in [(16000, 44101), (0, 16000), (16000, 0), (-48000, 16000), (16000, -1), (44100.5, 16000),
                (16000, 22050.25), (True, 16000), ("48000", 16000), (float("nan"), 16000), (float("inf"), 16000)]:
        with pytest.raises(ValueError):
            R.ratio(*bad)


def test_phase_table_and_tiles():
    from tinyrecurrentunet_amd import resample as R
    for p, q in RATIOS + [(1, 6), (6, 1), (80, 441), (441, 640)]:
        h, half = R.design(p, q)
        K = R.taps_per_output(p, half)
        assert K == -(-(2 * half + 1) // p) == RR.taps_per_output(p, half)
        tab = R.phase_table(h, p)
        Kp = tab.shape[1]
        assert tab.shape[0] == p and Kp % 4 == 0 and K <= Kp < K + 4 and tab.flags["C_CONTIGUOUS"]
        t = np.arange(p)[:, None] + p * np.arange(Kp)[None, :]
        assert np.array_equal(tab, np.where(t <= 2 * half, h[np.minimum(t, 2 * half)], 0.0))
    # every ratio the resampler accepts: the tile is a multiple of 256 and what a workgroup stages fits the declared budget;
    # a span that does not fit one window is staged in several (only for ratios far below 1)
    assert R.LDS_BUDGET <= 160 * 1024 and R.SPAN_FLOATS % 4 == 0
    # the limits the module lays its calls out by are the ones the kernels are built with
    with open(os.path.join(ROOT, "include", "trunet_hip.h")) as f:
        defines = {k: int(v) for k, v in re.findall(r"^#define TRUNET_RS_(\w+) (\d+)\b", f.read(), re.M)}
    assert defines == dict(MAX_TILE=R.MAX_TILE, SPAN_MAX=R.SPAN_FLOATS, TAPS_LDS_MAX=R.TAPS_LDS_FLOATS,
                           STREAM_INTS=R.STREAM_INTS, STREAM_MAX_HISTORY=R.MAX_HISTORY)
    for p in range(1, R.MAX_RATIO + 1):
        for q in range(1, R.MAX_RATIO + 1):
            if math.gcd(p, q) != 1 or p == q:
                continue
            tile = R.tile_outputs(p, q)
            assert tile % 256 == 0 and 256 <= tile <= R.MAX_TILE
            span = R.span_floats(p, q, tile)
            # the span covers every sample the tile's outputs read: first tap of the last output down to the last of the first
            half = 16 * max(p, q)
            K = R.taps_per_output(p, half)
            assert span >= ((tile - 1) * q + half) // p - half // p + K
            assert R.windows(p, q) == -(-span // R.SPAN_FLOATS)
            if tile > 256:
                assert span <= R.SPAN_FLOATS
            if tile < R.MAX_TILE:
                assert R.span_floats(p, q, tile + 256) > R.SPAN_FLOATS    # the largest tile that fits
            assert R.lds_bytes(p, q) <= R.LDS_BUDGET
            assert R.taps_in_lds(p, half) == (p * ((K + 3) // 4 * 4) <= R.TAPS_LDS_FLOATS)
    # the rates the module names run in one window: the whole span of a tile is in LDS at once
    for fs in RATES:
        for p, q in (R.ratio(fs, 16000), R.ratio(16000, fs)):
            assert R.windows(p, q) == 1 and 4 * R.span_floats(p, q, R.tile_outputs(p, q)) <= 4 * R.SPAN_FLOATS


def test_entry_point_rejects_null_and_bad_shapes():
    from tinyrecurrentunet_amd import _lib
    lib = _lib.lib()
    EINVAL = _lib.TRUNET_EINVAL
    rs = lib.trunet_resample_rational
    a, b, io, oo, to, t = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    # one utterance of 48000 samples at 48 kHz -> 16000: p = 1, q = 3, half = 48, K = 97, tile 1280 -> 13 tiles
    good = dict(inp=a, out=b, io=io, oo=oo, to=to, tab=t, half=48, K=97, p=1, q=3, tile=1280, B=1, nI=48000, nO=16000,
                nT=13, nsig=1, lds=1)

    def call(**kw):
        v = dict(good, **kw)
        return rs(v["inp"], v["out"], v["io"], v["oo"], v["to"], v["tab"], v["half"], v["K"], v["p"], v["q"], v["tile"],
                  v["B"], v["nI"], v["nO"], v["nT"], v["nsig"], v["lds"], None)

    for name in ("inp", "out", "io", "oo", "to", "tab"):
        assert call(**{name: None}) == EINVAL, name
    assert call(B=0) == EINVAL and call(B=-1) == EINVAL
    assert call(nsig=0) == EINVAL and call(nsig=3) == EINVAL
    assert call(p=0) == EINVAL and call(q=0) == EINVAL
    assert call(p=641, q=3, half=16 * 641, K=33) == EINVAL
    assert call(q=641, half=16 * 641, K=2 * 16 * 641 + 1) == EINVAL
    assert call(half=47) == EINVAL and call(half=0, K=1) == EINVAL          # half is a positive multiple of max(p, q)
    assert call(half=33 * 3, K=199) == EINVAL                               # more than 32 zero crossings
    assert call(K=96) == EINVAL and call(K=98) == EINVAL                    # K = ceil((2 half + 1) / p)
    assert call(tile=0) == EINVAL and call(tile=1000) == EINVAL and call(tile=8192) == EINVAL
    assert call(nI=-1) == EINVAL and call(nO=-1) == EINVAL and call(nT=-1) == EINVAL
    assert call(nO=16001) == EINVAL and call(nO=15999) == EINVAL            # not ceil(L p / q)
    assert call(nT=12) == EINVAL and call(nT=14) == EINVAL                  # not ceil(M / tile)
    assert call(nI=2 ** 31, nO=-(-2 ** 31 // 3)) == EINVAL                  # beyond int32 packing
    assert call(p=3, q=1, nI=2 ** 30, nO=3 * 2 ** 30, K=33, nT=-(-3 * 2 ** 30 // 1280)) == EINVAL
    assert call(lds=2) == EINVAL
    assert call(p=640, q=441, half=10240, K=33, nI=441, nO=640, nT=1, lds=1) == EINVAL     # a 92 KB table, LDS share 64 KB


def _stub_net():
    class Net:
        training, use_tgru = False, False
    return Net()


def test_host_side_refusals_before_any_launch():
    from tinyrecurrentunet_amd import _lib
    from tinyrecurrentunet_amd import resample as R
    from tinyrecurrentunet_amd.enhance import enhance
    ok = torch.zeros(4000)
    with pytest.raises(_lib.TrunetHipError):
        R.resample([ok, ok], 48000, 16000)                                  # CPU tensors
    with pytest.raises(_lib.TrunetHipError):
        R.resample(torch.zeros(2, 4000), 48000, 16000, lengths=[4000, 100])
    with pytest.raises(_lib.TrunetHipError):
        R.resample([ok], 16000, 16000)
    with pytest.raises(ValueError, match="lengths"):
        R.resample(torch.zeros(2, 4000), 48000, 16000, lengths=[4000, 4001])
    with pytest.raises(ValueError, match="lengths"):
        R.resample(torch.zeros(2, 4000), 48000, 16000, lengths=[4000])
    with pytest.raises(ValueError, match="lengths"):
        R.resample([ok], 48000, 16000, lengths=[4000])
    with pytest.raises(ValueError):
        R.resample([ok], 48000, 16001)
    with pytest.raises(ValueError, match="1-D"):
        R.resample([torch.zeros(2, 10)], 48000, 16000)
    # the plan of a call: an empty utterance, totals beyond int32 packing
    outs, offs = R.plan([3001, 1, 48000], 1, 3, 1280)
    assert outs == [1001, 1, 16000] and offs.dtype == np.int64
    assert offs.tolist() == [[0, 3001, 3002, 51002], [0, 1001, 1002, 17002], [0, 1, 2, 15]]
    with pytest.raises(ValueError, match="utterance 1 is empty"):
        R.plan([100, 0], 1, 3, 1280)
    with pytest.raises(ValueError, match="2\\^31"):
        R.plan([2 ** 30, 2 ** 30], 1, 3, 1280)
    with pytest.raises(ValueError, match="2\\^31"):
        R.plan([2 ** 30], 3, 1, 4096)
    # enhance(fs=...)
    net = _stub_net()
    with pytest.raises(_lib.TrunetHipError):
        enhance(net, [torch.zeros(48000)], fs=48000)                        # CPU tensors
    with pytest.raises(ValueError, match="lengths"):
        enhance(net, torch.zeros(2, 4000), lengths=[4000, 4001], fs=48000)
    with pytest.raises(ValueError, match="utterance 1 "):
        enhance(net, [torch.zeros(48000), torch.zeros(768)], fs=48000)      # 256 samples at 16 kHz
    with pytest.raises(ValueError, match="utterance 0 "):
        enhance(net, [torch.zeros(705)], fs=44100)                          # ceil(705 * 160 / 441) = 256
    with pytest.raises(_lib.TrunetHipError):
        enhance(net, [torch.zeros(706)], fs=44100)                          # 257 at 16 kHz: only the device is missing
    with pytest.raises(ValueError):
        enhance(net, [torch.zeros(48000)], fs=44101)


def _write_pairs(root, rate, n=2, length=6000):
    from scipy.io import wavfile
    os.makedirs(os.path.join(root, "clean"))
    os.makedirs(os.path.join(root, "keyboard"))
    g = np.random.default_rng(7)
    for i in range(n):
        wavfile.write(os.path.join(root, "clean", "fileid_%d.wav" % i), rate,
                      (8000 * g.standard_normal(length)).astype(np.int16))
    wavfile.write(os.path.join(root, "keyboard", "noise.wav"), rate, (3000 * g.standard_normal(length)).astype(np.int16))


def test_dataset_refuses_other_rates_and_a_reverb_at_the_wrong_rate(tmp_path):
    from tinyrecurrentunet_amd import dataset as ds
    root = str(tmp_path / "d")
    _write_pairs(root, 44100)
    with pytest.raises(ValueError, match="44100 Hz"):
        ds.CleanNoisyPairDataset(root, "training", 0, 48000, resample_to=16000)[0]
    item = ds.CleanNoisyPairDataset(root, "training", 0, 44100, resample_to=16000)[0]
    assert len(item) == 4 and item[0].shape == (1, 6000)                    # workers crop at the file rate
    plain = ds.CleanNoisyPairDataset(root, "training", 0, 48000)[0]        # without resample_to nothing is checked
    assert plain[0].shape == (1, 6000)
    with pytest.raises(ValueError, match="Reverb is built for 48000 Hz"):
        ds.CleanNoisyPairDataset(root, "training", 0, 48000, reverb=ds.Reverb(sample_rate=48000), resample_to=16000)
    ds.CleanNoisyPairDataset(root, "training", 0, 48000, reverb=ds.Reverb(sample_rate=16000), resample_to=16000)
    with pytest.raises(ValueError, match="no resampling"):
        ds.CleanNoisyPairDataset(root, "training", 0, 48000, reverb=ds.Reverb(sample_rate=16000))
    with pytest.raises(ValueError):
        ds.CleanNoisyPairDataset(root, "training", 0, 48000, resample_to=16001)
    with pytest.raises(ValueError, match="Reverb is built for 48000 Hz"):
        ds.load_CleanNoisyPairDataset(root, "training", 0, 2, 48000, num_workers=0, reverb=ds.Reverb(sample_rate=48000),
                                      resample_to=16000)
    assert "48 kHz" in ds.DataAugment.__doc__


def test_enhance_command_line_mentions_resample():
    r = subprocess.run([sys.executable, "-m", "tinyrecurrentunet_amd.enhance", "--help"], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    text = " ".join(r.stdout.split())
    assert "--resample" in text and "above 8 kHz is not restored" in text
