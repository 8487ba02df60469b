"""GPU: the rational resampler (tinyrecurrentunet_amd/resample.py, resample.hip) -- the kernel against
the float64 restatement within the derived rounding bound at the kernel's edges, bit-for-bit independence of batch-mates,
order, input form and plane, the identity, enhance(fs=...), the command line's --resample and the loader's resample_to."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import resample_ref as RR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ratio -> the input rate it stands for next to the network's 16 kHz
RATIOS = {(1, 3): 48000, (3, 1): 16000, (2, 1): 8000, (1, 2): 32000, (1, 6): 96000, (160, 441): 44100, (441, 160): 16000,
          (640, 441): 11025}
# ratios far below 1, whose span is staged in several windows (the kernel's other path); short utterances only
WINDOWED = {(1, 40): 16000, (7, 160): 16000}


def _signal(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def _check_case(x, y, p, q, h=None):
    """one utterance: the fp32 result y against the restatement on the fp32 samples and float64 taps -> |err| / bound max"""
    ref, a = RR.resample(x.astype(np.float64), p, q, h)
    half = 16 * max(p, q) if h is None else (len(h) - 1) // 2
    assert y.shape == ref.shape, (p, q, x.shape, y.shape, ref.shape)
    bound = RR.bound(a, p, half)
    err = np.abs(y.astype(np.float64) - ref)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    assert np.all(err <= bound), (p, q, x.shape[0], worst, int(np.argmax(err / np.maximum(bound, 1e-300))))
    return worst


@pytest.mark.parametrize("pq", list(RATIOS) + list(WINDOWED))
def test_kernel_matches_the_restatement(pq):
    from tinyrecurrentunet_amd import resample as R
    p, q = pq
    fs_in = RATIOS.get(pq) or WINDOWED[pq]
    fs_out = fs_in * p // q
    assert R.ratio(fs_in, fs_out) == (p, q)
    tile = R.tile_outputs(p, q)
    if pq in WINDOWED:
        assert R.windows(p, q) > 1
        outs = [1, 2, 255, 256, 257, 600]
        long_in = 0
    else:
        assert R.windows(p, q) == 1
        outs = [1, 2, 255, 256, 257, tile - 1, tile, tile + 1, 2 * tile + 17]
        long_in = 3 * fs_in                              # one utterance of 3 s shares the batch
    lens = [-(-m * q // p) for m in outs] + ([long_in] if long_in else [])
    xs = [_signal(n, 100 * p + q + i) for i, n in enumerate(lens)]
    ys = R.resample([torch.from_numpy(x).cuda() for x in xs], fs_in, fs_out)
    torch.cuda.synchronize()
    worst = 0.0
    for x, y in zip(xs, ys):
        assert y.dtype == torch.float32 and y.shape == (R.out_length(x.shape[0], p, q),)
        worst = max(worst, _check_case(x, y.cpu().numpy(), p, q))
    print("resample %d/%d: tile %d, largest |err| / bound = %.4f" % (p, q, tile, worst))


def test_taps_from_l2_and_from_lds_agree_bit_for_bit():
    """the tap table in LDS or read from L2 is a choice of speed: same taps, same order, same bits"""
    from tinyrecurrentunet_amd import resample as R
    lens = [1, 5000, 44100]
    xs = [torch.from_numpy(_signal(n, 40 + n)).cuda() for n in lens]
    for fs_in, fs_out in ((44100, 16000), (16000, 44100), (48000, 16000)):
        a = R.Resampler(fs_in, fs_out, "cuda", lds_taps=True)(xs)
        b = R.Resampler(fs_in, fs_out, "cuda", lds_taps=False)(xs)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    with pytest.raises(ValueError, match="LDS"):
        R.Resampler(11025, 16000, "cuda", lds_taps=True)


@pytest.mark.parametrize("rates", [(48000, 16000), (44100, 16000), (16000, 44100), (11025, 16000)])
def test_each_utterance_is_independent_of_the_batch_bit_for_bit(rates):
    from tinyrecurrentunet_amd import resample as R
    fs_in, fs_out = rates
    p, q = R.ratio(fs_in, fs_out)
    tile = R.tile_outputs(p, q)
    lens = [1, 257, -(-tile * q // p), -(-(tile + 1) * q // p) + 3, 20011]
    xs = [torch.from_numpy(_signal(n, 7 * n + p)).cuda() for n in lens]
    alone = [R.resample([x], fs_in, fs_out)[0] for x in xs]
    batch = R.resample(xs, fs_in, fs_out)
    again = R.resample(xs, fs_in, fs_out)
    perm = [3, 0, 4, 2, 1]
    permuted = R.resample([xs[i] for i in perm], fs_in, fs_out)
    width = max(lens) + 5
    X = torch.full((len(xs), width), 7.0, device="cuda")           # what lies past a length must not matter
    for b, x in enumerate(xs):
        X[b, :lens[b]] = x
    padded = R.resample(X, fs_in, fs_out, lengths=lens)
    assert padded.shape == (len(xs), R.out_length(width, p, q))
    rs = R.Resampler(fs_in, fs_out, "cuda")
    other = [torch.from_numpy(_signal(n, 13 * n + q)).cuda() for n in lens]
    p0, p1 = rs(xs, x2=other)
    o0, o1 = rs(other, x2=xs)
    for b in range(len(xs)):
        m = R.out_length(lens[b], p, q)
        assert alone[b].shape == (m,)
        assert torch.equal(alone[b], batch[b]) and torch.equal(batch[b], again[b])
        assert torch.equal(alone[b], permuted[perm.index(b)])
        assert torch.equal(alone[b], padded[b, :m]) and not padded[b, m:].any()
        assert torch.equal(alone[b], p0[b]) and torch.equal(alone[b], o1[b])
        assert torch.equal(p1[b], o0[b]) and torch.equal(p1[b], R.resample([other[b]], fs_in, fs_out)[0])
    # the rows form the loader uses: (nsig, B, L)
    rows = torch.stack([torch.stack([xs[4], other[4]]), torch.stack([other[4], xs[4]])])
    y = rs.rows(rows)
    assert torch.equal(y[0, 0], alone[4]) and torch.equal(y[1, 1], alone[4]) and torch.equal(y[0, 1], y[1, 0])


def test_identity_returns_equal_tensors_that_do_not_alias():
    from tinyrecurrentunet_amd import resample as R
    xs = [torch.from_numpy(_signal(n, n)).cuda() for n in (1, 1000)]
    ys = R.resample(xs, 16000, 16000)
    for x, y in zip(xs, ys):
        assert torch.equal(x, y) and y.data_ptr() != x.data_ptr()
    X = torch.from_numpy(_signal(2000, 5)).cuda().view(2, 1000)
    Y = R.resample(X, 44100, 44100, lengths=[1000, 10])
    assert Y.data_ptr() != X.data_ptr() and torch.equal(Y[0], X[0]) and torch.equal(Y[1, :10], X[1, :10])
    assert not Y[1, 10:].any()


_NETS = {}


def _net(cin):
    from oracle import network_ref as nr, weights as W
    from tinyrecurrentunet_amd import network as hn
    if cin not in _NETS:
        net = hn.TRUNet(input_size=cin)
        net.load_state_dict(W.fill_state_dict(nr.TRUNet(input_size=cin), seed=5).state_dict())
        _NETS[cin] = net.cuda().eval()
    return _NETS[cin]


@pytest.mark.parametrize("cin", [3, 4])
@pytest.mark.parametrize("fs", [48000, 44100])
def test_enhance_at_another_rate_is_the_composition(cin, fs):
    from tinyrecurrentunet_amd import resample as R
    from tinyrecurrentunet_amd.enhance import enhance
    net = _net(cin)
    lens = [12345, 48000, 50001]
    xs = [torch.from_numpy(0.1 * _signal(n, n + cin)).cuda() for n in lens]
    ys = enhance(net, xs, fs=fs)
    down = R.resample(xs, fs, 16000)
    up = R.resample(enhance(net, down), 16000, fs)
    for x, y, u in zip(xs, ys, up):
        assert y.shape == x.shape and u.shape[0] >= x.shape[0]
        assert torch.equal(y, u[:x.shape[0]])
        assert torch.isfinite(y).all()
    # the padded form: the same bits, zeros past each length
    width = max(lens) + 3
    X = torch.zeros((3, width), device="cuda")
    for b, x in enumerate(xs):
        X[b, :lens[b]] = x
    Y = enhance(net, X, lengths=lens, fs=fs)
    assert Y.shape == X.shape
    for b, n in enumerate(lens):
        assert torch.equal(Y[b, :n], ys[b]) and not Y[b, n:].any()
    # the default rate: the call without fs
    for a, b in zip(enhance(net, xs, fs=16000), enhance(net, xs)):
        assert torch.equal(a, b)


def test_command_line_resamples_each_file_back_to_its_rate(tmp_path):
    from scipy.io.wavfile import read as wavread, write as wavwrite
    net = _net(4)
    ind, outd = tmp_path / "noisy", tmp_path / "out"
    ind.mkdir()
    g = np.random.default_rng(91)
    files = {"a16.wav": (16000, 9000), "b44.wav": (44100, 30001), "c48.wav": (48000, 24000)}
    for nm, (sr, n) in files.items():
        wavwrite(str(ind / nm), sr, (g.standard_normal(n) * 3000).astype(np.int16))
    ck = tmp_path / "ck.pkl"
    torch.save({"iter": 1, "model_state_dict": {k: v.cpu() for k, v in net.state_dict().items()}}, str(ck))
    cmd = [sys.executable, "-m", "tinyrecurrentunet_amd.enhance", "--checkpoint", str(ck), "--input-size", "4", "--in",
           str(ind), "--out", str(outd)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "the network runs at 16000 Hz (no resampling)" in r.stderr, r.stdout + r.stderr
    r = subprocess.run(cmd + ["--resample", "--max-seconds", "0.7"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(outd)) == sorted(files)
    for nm, (sr, n) in files.items():
        sr_out, q = wavread(str(outd / nm))
        assert sr_out == sr and q.dtype == np.int16 and q.shape == (n,), nm
        assert np.abs(q.astype(np.int64)).max() > 0, nm


def test_loader_resamples_both_signals_before_the_mix(tmp_path):
    from scipy.io.wavfile import write as wavwrite
    from tinyrecurrentunet_amd import dataset as ds
    n, sr = 20001, 48000
    (tmp_path / "clean").mkdir()
    (tmp_path / "keyboard").mkdir()
    g = np.random.default_rng(17)
    clean = [(g.standard_normal(n) * 3000).astype(np.int16) for _ in range(3)]
    for i, c in enumerate(clean):
        wavwrite(str(tmp_path / "clean" / ("fileid_%d.wav" % i)), sr, c)
    wavwrite(str(tmp_path / "keyboard" / "k0.wav"), sr, (g.standard_normal(n) * 1000).astype(np.int16))

    def batches(**kw):
        random.seed(3)
        np.random.seed(3)
        torch.manual_seed(3)
        loader = ds.load_CleanNoisyPairDataset(root=str(tmp_path), subset="training", crop_length_sec=0, batch_size=3,
                                               sample_rate=sr, num_workers=0, **kw)
        out = [(c.clone(), y.clone(), list(f)) for c, y, f in loader]
        torch.cuda.synchronize()
        return out

    (c16, y16, ids), = batches(resample_to=16000)
    m = -(-n // 3)
    assert c16.shape == (3, 1, m) and y16.shape == c16.shape and c16.is_cuda and y16.is_cuda
    for b, fid in enumerate(ids):
        i = int(os.path.basename(fid)[len("fileid_"):-len(".wav")])
        x = clean[i].astype(np.float32) / 32768.0
        worst = _check_case(x, c16[b, 0].cpu().numpy(), 1, 3)
        print("loader clean %d: largest |err| / bound = %.4f" % (i, worst))
    assert float((y16 - c16).abs().max()) > 0                               # the noise was mixed in at 16 kHz
    # the reverberation stage takes the resampled pair: a Reverb built for 16 kHz, output at 16 kHz
    (t16, r16, _), = batches(resample_to=16000, reverb=ds.Reverb(sample_rate=16000, p_reverb=1.0, max_rir_sec=0.2),
                             snr_db=(5.0, 5.0))
    assert t16.shape == (3, 1, m) and r16.shape == t16.shape and torch.isfinite(r16).all() and float(r16.abs().max()) > 0
    # without resample_to: exactly the batch of a loader that was never given the keyword, the files' own samples
    (c0, y0, ids0), = batches(resample_to=None)
    (c1, y1, ids1), = batches()
    assert ids0 == ids1 and torch.equal(c0, c1) and torch.equal(y0, y1) and c0.shape == (3, 1, n)
    for b, fid in enumerate(ids0):
        i = int(os.path.basename(fid)[len("fileid_"):-len(".wav")])
        assert np.array_equal(c0[b, 0].cpu().numpy(), clean[i].astype(np.float32) / 32768.0)
