"""GPU: the band above 8 kHz around a 16 kHz enhancement (tinyrecurrentunet_amd/highband.py, highband.hip; DESIGN section
3p) -- the gains and the join kernels against the float64 restatement (tests/highband_ref.py) within derived rounding
bounds at the kernels' edges, the exact cases, utterances the kernels must skip, bit-for-bit independence of batch-mates,
order and input form, and the modes through enhance() and the command line.

Largest |err| / bound observed on the MI355X:
    gains          0.0026  (a worst-case bound over 63 taps and 512 squares)
    join "keep"    0.25    (1/3 0.234, 160/441 0.230, 1/2 0.222, 1/6 0.248)
    join "follow"  0.37    (1/3 0.369, 160/441 0.359, 1/2 0.318, 1/6 0.328)"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import highband_ref as HR
import resample_ref as RR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24
# 16000 / fs in lowest terms -> fs
RATIOS = {(1, 3): 48000, (160, 441): 44100, (1, 2): 32000, (1, 6): 96000}


def _signal(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def _slow(n, seed):
    """a slowly varying factor in [0, 1.5]"""
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.75 + 0.75 * np.sin(2 * np.pi * g.uniform(2.0, 9.0) * t + g.uniform(0, 6.0))).astype(np.float32)


def _cuda(xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def test_gains_match_the_restatement():
    """Gaussian lo, y16 = lo m with a slowly varying m in [0, 1.5]; one batch with the shortest utterances, those around a
    hop-block boundary, those around one workgroup's span and 0.3 s; |g - g_ref| <= the bound highband_ref.gains derives"""
    from tinyrecurrentunet_amd import highband as HB
    span = HB.RUN * HB.HOP
    lens = [257, 383, 384, 385, span - 1, span, span + 1, 4803]
    lo = [_signal(n, 11 * n) for n in lens]
    y16 = [x * _slow(n, n) for x, n in zip(lo, lens)]
    gs = HB.gains(_cuda(lo), _cuda(y16))
    torch.cuda.synchronize()
    g_min = HB.floor_gain(-30.0)
    worst = 0.0
    for x, y, g, n in zip(lo, y16, gs, lens):
        assert g.dtype == torch.float32 and g.shape == (1 + n // 128,)
        ref, bound = HR.gains(x.astype(np.float64), y.astype(np.float64), g_min=g_min)
        err = np.abs(g.cpu().numpy().astype(np.float64) - ref)
        ratio = float(np.max(err / bound))
        print("gains L16 = %d: largest |err| / bound = %.4f (bound at most %.2e)" % (n, ratio, bound.max()))
        assert np.all(err <= bound), (n, ratio, int(np.argmax(err / bound)))
        assert g_min <= float(g.min()) and float(g.max()) <= 1.0
        worst = max(worst, ratio)
    print("gains: largest |err| / bound = %.4f" % worst)


def test_gains_exact_cases():
    from tinyrecurrentunet_amd import highband as HB
    lens = [257, 2049, 4803]
    lo = _cuda([_signal(n, 3 * n) for n in lens])
    quarter = HB.gains(lo, [0.25 * x for x in lo])
    zeros = [torch.zeros_like(x) for x in lo]
    silent = HB.gains(zeros, zeros)
    removed = HB.gains(lo, zeros)
    deeper = HB.gains(lo, zeros, floor_db=-60.0)
    for q, s, r, d in zip(quarter, silent, removed, deeper):
        assert float((q - 0.25).abs().max()) <= 2 * 2.0 ** -25                # 2 ulp of 0.25
        assert torch.equal(s, torch.ones_like(s))
        assert torch.equal(r, torch.full_like(r, HB.floor_gain(-30.0)))
        assert torch.equal(d, torch.full_like(d, HB.floor_gain(-60.0)))


def _join_bound(up_y, up_x, x, G):
    """three roundings of the sum and three of the interpolation, with or without fused multiply-add"""
    return 4 * U32 * np.abs(up_y) + 8 * U32 * G * (np.abs(x) + np.abs(up_x))


def _lengths(pd, qd, fs):
    first = 256 * qd // pd + 1                          # the shortest with ceil(L pd / qd) = 257
    return [first, first + 1, 2 * 4096 + 3, int(0.3 * fs) + 1]


@pytest.mark.parametrize("mode", ["keep", "follow"])
@pytest.mark.parametrize("pq", list(RATIOS))
def test_join_matches_float64(pq, mode):
    """rejoin against up_y + G (x - up_x) in float64, computed from the fp32 up_y and up_x of the same resampler, the same x
    and the kernel's own g; the lengths put the utterances at every alignment of the packed buffers"""
    from tinyrecurrentunet_amd import highband as HB, resample as R
    pd, qd = pq
    fs = RATIOS[pq]
    assert R.ratio(fs, 16000) == pq
    lens = _lengths(pd, qd, fs)
    assert R.out_length(lens[0], pd, qd) == 257 and R.out_length(lens[0] - 1, pd, qd) == 256 and lens[2] % 4
    xs = _cuda([_signal(n, 5 * n + pd) for n in lens])
    lo = R.resample(xs, fs, 16000)
    y16 = [v * torch.from_numpy(_slow(v.shape[0], 17 * n)).cuda() for v, n in zip(lo, lens)]
    out = HB.rejoin(xs, lo, y16, fs, mode)
    up_y, up_x = R.resampler(16000, fs, "cuda")(y16, x2=lo)
    gs = HB.gains(lo, y16)
    torch.cuda.synchronize()
    worst = 0.0
    for x, o, uy, ux, g, n in zip(xs, out, up_y, up_x, gs, lens):
        assert o.dtype == torch.float32 and o.shape == (n,) and uy.shape[0] >= n
        x, uy, ux = (v.cpu().numpy().astype(np.float64)[:n] for v in (x, uy, ux))
        G = HR.sample_gains(g.cpu().numpy().astype(np.float64), n, pd, qd) if mode == "follow" else np.ones(n)
        ref = HR.join(uy, ux, x, G)
        bound = _join_bound(uy, ux, x, G)
        err = np.abs(o.cpu().numpy().astype(np.float64) - ref)
        ratio = float(np.max(err / np.maximum(bound, 1e-300)))
        assert np.all(err <= bound), (pq, mode, n, ratio, int(np.argmax(err / np.maximum(bound, 1e-300))))
        worst = max(worst, ratio)
    print("join %d/%d %s: largest |err| / bound = %.4f" % (pd, qd, mode, worst))
    # "drop" through the same call: the resampled enhancement, cut
    for d, uy, n in zip(HB.rejoin(xs, lo, y16, fs, "drop"), up_y, lens):
        assert torch.equal(d, uy[:n])


def test_utterances_with_contradicting_offsets_are_skipped():
    """what the host cannot see: a frame table, or an upsampled extent, that does not fit an utterance's samples.  The
    kernels leave that utterance's outputs alone and serve the others; every access stays inside the declared totals."""
    from tinyrecurrentunet_amd import _lib, highband as HB
    lib, st = _lib.lib(), _lib.stream()
    L0, L1 = 257, 300
    lo = torch.from_numpy(_signal(L0 + L1, 1)).cuda()
    y16 = 0.5 * lo
    good = HB.gains([lo[:L0]], [y16[:L0]])[0]
    offs = torch.tensor([[0, L0, L0 + L1], [0, 3, 5]], dtype=torch.int64).cuda()      # utterance 1 has 3 frames, not 2
    g = torch.full((5,), -7.0, device="cuda")
    energy = torch.empty((5, 2), device="cuda")
    rc = lib.trunet_highband_gains(lo.data_ptr(), y16.data_ptr(), offs[0].data_ptr(), offs[1].data_ptr(),
                                   HB._taps(lo.device).data_ptr(), energy.data_ptr(), g.data_ptr(), 2, L0 + L1, 5,
                                   HB.floor_gain(-30.0), st)
    assert rc == 0
    assert torch.equal(g[:3], good) and torch.equal(g[3:], torch.full((2,), -7.0, device="cuda"))
    # the join: utterance 1 would need 300 upsampled samples and its table offers 299
    n = L0 + L1
    up_y, up_x, x = (torch.from_numpy(_signal(n, s)).cuda() for s in (2, 3, 4))
    so = torch.tensor([[0, L0, n], [0, L0 + 1, n]], dtype=torch.int64).cuda()
    out = torch.full((n,), -7.0, device="cuda")
    rc = lib.trunet_highband_join(up_y.data_ptr(), up_x.data_ptr(), x.data_ptr(), None, out.data_ptr(), so[0].data_ptr(),
                                  so[1].data_ptr(), None, 2, n, n, 0, 1, 3, HB.KEEP, st)
    assert rc == 0
    assert torch.equal(out[:L0], up_y[:L0] + (x[:L0] - up_x[:L0]))
    assert torch.equal(out[L0:], torch.full((L1,), -7.0, device="cuda"))


@pytest.mark.parametrize("fs", [48000, 44100])
def test_each_utterance_is_independent_of_the_batch_bit_for_bit(fs):
    from tinyrecurrentunet_amd import highband as HB, resample as R
    pd, qd = R.ratio(fs, 16000)
    lens = [256 * qd // pd + 1, 4099, 2 * 4096 + 3, int(0.3 * fs) + 2, 6 * 2048 * qd // pd + 5]
    xs = _cuda([_signal(n, 7 * n + 1) for n in lens])
    lo = R.resample(xs, fs, 16000)
    y16 = [v * torch.from_numpy(_slow(v.shape[0], n)).cuda() for v, n in zip(lo, lens)]
    perm = [3, 0, 4, 2, 1]
    for mode in ("keep", "follow"):
        alone = [HB.rejoin([x], [a], [b], fs, mode)[0] for x, a, b in zip(xs, lo, y16)]
        batch = HB.rejoin(xs, lo, y16, fs, mode)
        again = HB.rejoin(xs, lo, y16, fs, mode)
        permuted = HB.rejoin([xs[i] for i in perm], [lo[i] for i in perm], [y16[i] for i in perm], fs, mode)
        for b in range(len(xs)):
            assert alone[b].shape == xs[b].shape
            assert torch.equal(alone[b], batch[b]) and torch.equal(batch[b], again[b])
            assert torch.equal(alone[b], permuted[perm.index(b)])
    g_alone = [HB.gains([a], [b])[0] for a, b in zip(lo, y16)]
    for u, v in zip(g_alone, HB.gains(lo, y16)):
        assert torch.equal(u, v)


_NETS = {}


def _net(cin=4):
    from oracle import network_ref as nr, weights as W
    from tinyrecurrentunet_amd import network as hn
    if cin not in _NETS:
        net = hn.TRUNet(input_size=cin)
        net.load_state_dict(W.fill_state_dict(nr.TRUNet(input_size=cin), seed=5).state_dict())
        _NETS[cin] = net.cuda().eval()
    return _NETS[cin]


def _amplitude(v, f0, fs):
    """amplitude of the sine at f0 by projection over the middle half"""
    n = np.arange(v.shape[0])
    m = slice(v.shape[0] // 4, 3 * v.shape[0] // 4)
    return 2.0 * np.abs(np.sum(v[m].astype(np.float64) * np.exp(-2j * np.pi * f0 * n[m] / fs))) / (m.stop - m.start)


@pytest.mark.parametrize("fs", [48000, 44100])
def test_enhance_modes(fs):
    """three utterances of 0.1 to 0.3 s through enhance(): "drop" is the call without the argument, "keep" - "drop" is
    x - U(D(x)), the padded form has the list's bits, and a 12 kHz tone is lost by "drop" and returned by "keep" """
    from tinyrecurrentunet_amd import resample as R
    from tinyrecurrentunet_amd.enhance import enhance
    net = _net()
    lens = [int(0.1 * fs) + 1, int(0.2 * fs) + 2, int(0.3 * fs)]
    tone = 0.1 * np.sin(2 * np.pi * 12000.0 * np.arange(lens[2]) / fs + 0.3)
    sig = [0.1 * _signal(n, n + 3) for n in lens]
    spec = np.fft.rfft(sig[2])
    spec[int(3000.0 * lens[2] / fs):] = 0.0                                  # the third: noise below 3 kHz + the tone
    sig[2] = (np.fft.irfft(spec, lens[2]) + tone).astype(np.float32)
    xs = _cuda(sig)
    plain = enhance(net, xs, fs=fs)
    drop = enhance(net, xs, fs=fs, highband="drop")
    keep = enhance(net, xs, fs=fs, highband="keep")
    follow = enhance(net, xs, fs=fs, highband="follow", highband_floor_db=-40.0)
    up_x = R.resample(R.resample(xs, fs, 16000), 16000, fs)
    torch.cuda.synchronize()
    for x, a, d, k, f, ux in zip(xs, plain, drop, keep, follow, up_x):
        assert torch.equal(a, d)
        assert k.shape == f.shape == x.shape and torch.isfinite(k).all() and torch.isfinite(f).all()
        x, d, k, f, ux = (v.cpu().numpy().astype(np.float64)[:x.shape[0]] for v in (x, d, k, f, ux))
        assert np.all(np.abs((k - d) - (x - ux)) <= _join_bound(d, ux, x, 1.0))
        # "follow" lies between "drop" and "keep": G in [g_min, 1] of the same band
        assert np.all(np.abs(f - d) <= np.abs(x - ux) * (1 + 8 * U32) + 4 * U32 * np.abs(d))
    a_drop, a_keep = _amplitude(drop[2].cpu().numpy(), 12000.0, fs), _amplitude(keep[2].cpu().numpy(), 12000.0, fs)
    print("12 kHz at %d Hz: drop %.3e, keep %.6f" % (fs, a_drop, a_keep))
    assert a_drop < 1e-3 * 0.1
    assert abs(a_keep - 0.1) <= 0.01 * 0.1
    # the padded form: the same bits, zeros past each length
    width = max(lens) + 3
    X = torch.zeros((3, width), device="cuda")
    for b, x in enumerate(xs):
        X[b, :lens[b]] = x
    for mode, want in (("keep", keep), ("follow", follow)):
        Y = enhance(net, X, lengths=lens, fs=fs, highband=mode, highband_floor_db=-40.0)
        assert Y.shape == X.shape
        for b, n in enumerate(lens):
            assert torch.equal(Y[b, :n], want[b]) and not Y[b, n:].any()


@pytest.mark.parametrize("fs", [16000, 8000])
def test_enhance_at_or_below_16k_has_no_band_to_keep(fs):
    from tinyrecurrentunet_amd.enhance import enhance
    net = _net()
    xs = _cuda([0.1 * _signal(n, n) for n in (int(0.1 * fs) + 1, int(0.3 * fs))])
    drop = enhance(net, xs, fs=fs)
    for mode in ("keep", "follow"):
        for a, b in zip(drop, enhance(net, xs, fs=fs, highband=mode)):
            assert torch.equal(a, b)


def test_command_line_highband_follow(tmp_path):
    from scipy.io.wavfile import read as wavread, write as wavwrite
    net = _net()
    ind, outd = tmp_path / "noisy", tmp_path / "out"
    ind.mkdir()
    g = np.random.default_rng(92)
    files = {"a16.wav": (16000, 5000), "b44.wav": (44100, 9001), "c48.wav": (48000, 12000)}
    noisy = {nm: (g.standard_normal(n) * 3000).astype(np.int16) for nm, (sr, n) in files.items()}
    for nm, (sr, n) in files.items():
        wavwrite(str(ind / nm), sr, noisy[nm])
    ck = tmp_path / "ck.pkl"
    torch.save({"iter": 1, "model_state_dict": {k: v.cpu() for k, v in net.state_dict().items()}}, str(ck))
    cmd = [sys.executable, "-m", "tinyrecurrentunet_amd.enhance", "--checkpoint", str(ck), "--input-size", "4", "--in",
           str(ind), "--out", str(outd), "--resample", "--highband", "follow", "--highband-floor-db", "-20"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(outd)) == sorted(files)
    for nm, (sr, n) in files.items():
        sr_out, q = wavread(str(outd / nm))
        assert sr_out == sr and q.dtype == np.int16 and q.shape == (n,), nm
        assert np.abs(q.astype(np.int64)).max() > 0, nm
    # G >= 10^(-20 / 20): from 10 kHz up the 48 kHz file keeps at least about a hundredth of its input's energy (half of
    # that asked for here); "drop" would leave less than a millionth
    band = lambda v: np.sum(np.abs(np.fft.rfft(v.astype(np.float64))[int(10000 * 12000 / 48000):]) ** 2)
    assert band(wavread(str(outd / "c48.wav"))[1]) >= 0.5 * 0.01 * band(noisy["c48.wav"])
