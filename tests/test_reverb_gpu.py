"""GPU: the reverberation stage (reverb.hip, dataset.Reverb, the loader keywords) against its float64 statement
(tests/reverb_ref.py).  Bound of every comparison with a convolution in it: per row, max|got - ref| / max|ref| over every
sample is at most 8x the same statistic of the reference's own fp32 partitioned restatement on the same inputs (the LDS
Stockham transform uses fp32 twiddle tables and sums partitions in another order than pocketfft), and never above 2e-5, the
project's bound for the augmentation stage."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reverb_ref as rr  # noqa: E402
from tinyrecurrentunet_amd import _lib  # noqa: E402
from tinyrecurrentunet_amd import dataset as ds  # noqa: E402

pytestmark = pytest.mark.gpu

SR = 16000
CAP = 2e-5


def _log(msg):
    """print a measured figure; with TRUNET_PARITY_DIR set to a folder, also append it to parity_reverb.txt there"""
    print(msg)
    out_dir = os.environ.get("TRUNET_PARITY_DIR")
    if out_dir and os.path.isdir(out_dir):
        open(os.path.join(out_dir, "parity_reverb.txt"), "a").write(msg + "\n")


def _rir(seed, k):
    """k taps of a synthetic RIR with rt60 between 0.2 and 1.2 s"""
    rt60 = min(max(k / SR + 0.05, 0.2), 1.2)
    h = ds.Reverb(sample_rate=SR, max_rir_sec=1.2).synthetic(seed, rt60, 3.0 + seed % 7)
    assert len(h) >= k
    return h[:k].astype(np.float32)


def _signals(B, Ln, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal((B, Ln))).astype(np.float32)


def run(clean, rirs, noise=None, snr=None, E=0, peak=0.99, kmax=None, pad=0.0):
    """trunet_reverb_mix on numpy inputs -> (noisy, target) as numpy; rirs: list of 1-D arrays (empty: no reverberation)
    or None; the (B, Kmax) array is padded with ``pad`` beyond each row's taps"""
    lib = _lib.lib()
    dev = torch.device("cuda")
    B, Ln = clean.shape
    c = torch.from_numpy(clean).to(dev)
    v = None if noise is None else torch.from_numpy(noise).to(dev)
    s = None if snr is None else torch.tensor(snr, dtype=torch.float32, device=dev)
    r = lens = ws = None
    K = nbytes = 0
    if rirs is not None:
        K = kmax or max(max(len(h) for h in rirs), 1)
        host = np.full((B, K), pad, dtype=np.float32)
        for b, h in enumerate(rirs):
            host[b, :len(h)] = h
        r = torch.from_numpy(host).to(dev)
        lens = torch.tensor([len(h) for h in rirs], dtype=torch.int32, device=dev)
        nbytes = lib.trunet_reverb_workspace_bytes(B, Ln, K)
        assert nbytes > 0
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)      # scratch: stale content must not matter
    noisy, target = torch.full_like(c, float("nan")), torch.full_like(c, float("nan"))
    rc = lib.trunet_reverb_mix(_lib.ptr(c), _lib.ptr(v), _lib.ptr(r), None if lens is None else lens.data_ptr(), _lib.ptr(s),
                               E, peak, _lib.ptr(noisy), _lib.ptr(target), None if ws is None else ws.data_ptr(), nbytes,
                               B, Ln, K, _lib.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return noisy.cpu().numpy(), target.cpu().numpy()


def _bound(x, h):
    """8x the reference's own fp32 error on this row, capped"""
    return min(8.0 * float(rr.rel_err(rr.conv32_partitioned(x, h), rr.conv64(x, h))[0]), CAP)


CONV_SHAPES = [
    (3, 3000, (1, 1024, 1025)),                    # a partition boundary on either side
    (2, 257, (700, 5000)),                         # an RIR longer than the signal, less than one block
    (4, 2048, (2, 1023, 2048, 2049)),              # block edges
    (5, 32000, (300, 1500, 4097, 8000, 12000)),    # ragged partition counts in one grid
    (1, 1, (1,)),                                  # one sample, one tap
    (2, 64000, (16000, 16000)),                    # one workload-sized case
]


@pytest.mark.parametrize("B,Ln,taps", CONV_SHAPES, ids=["%dx%d" % (b, l) for b, l, _ in CONV_SHAPES])
def test_convolution_matches_float64(B, Ln, taps):
    x = _signals(B, Ln, seed=Ln)
    hs = [_rir(10 + i, k) for i, k in enumerate(taps)]
    wet, tgt = run(x, hs, E=0, peak=0.0)
    assert np.array_equal(tgt, x)                                        # dry target, no rescale: bit for bit
    for b in range(B):
        ref = rr.conv64(x[b], hs[b])
        err = float(rr.rel_err(wet[b], ref)[0])
        bound = _bound(x[b], hs[b])
        _log("reverb conv B=%d L=%d taps=%d: err %.3e  bound %.3e (8 x the reference's fp32 restatement)"
             % (B, Ln, taps[b], err, bound))
        assert err <= bound, (B, Ln, taps[b], err, bound)


@pytest.mark.parametrize("E", [1, 800, 1024, 1500])
def test_early_target_matches_float64(E):
    x = _signals(2, 6000, seed=3)
    hs = [_rir(21, 5000), _rir(22, 1200)]                                # the second RIR ends before 1500 taps
    wet, tgt = run(x, hs, E=E, peak=0.0)
    for b in range(2):
        he = hs[b][:min(E, len(hs[b]))]
        err = float(rr.rel_err(tgt[b], rr.conv64(x[b], he))[0])
        bound = _bound(x[b], he)
        errw = float(rr.rel_err(wet[b], rr.conv64(x[b], hs[b]))[0])
        _log("reverb early E=%d taps=%d: target err %.3e bound %.3e; wet err %.3e" % (E, len(hs[b]), err, bound, errw))
        assert err <= bound, (E, b, err, bound)
        assert errw <= _bound(x[b], hs[b])


def test_rows_are_independent_and_padding_is_not_read():
    B, Ln = 5, 5000
    x = _signals(B, Ln, seed=5)
    v = 0.5 * _signals(B, Ln, seed=6)
    hs = [np.zeros(0, np.float32), _rir(31, 700), np.zeros(0, np.float32), _rir(32, 3000), _rir(33, 1025)]
    snr = [3.0, 7.0, 11.0, -2.0, 15.0]
    wet, tgt = run(x, hs, E=800, peak=0.0, pad=float("nan"))             # no noise, no guard: wet itself
    assert np.isfinite(wet).all() and np.isfinite(tgt).all()
    for b in (0, 2):
        assert np.array_equal(wet[b], x[b]) and np.array_equal(tgt[b], x[b])      # K_b = 0: the dry signal, bit for bit
    noisy, tgt = run(x, hs, noise=v, snr=snr, E=800, peak=0.99, pad=float("nan"))
    assert np.isfinite(noisy).all() and np.isfinite(tgt).all()
    noisy0, tgt0 = run(x, hs, noise=v, snr=snr, E=800, peak=0.99, pad=0.0, kmax=4096)
    assert np.array_equal(noisy, noisy0) and np.array_equal(tgt, tgt0)   # neither the padding nor Kmax reaches the output
    for b in range(B):
        alone = run(x[b:b + 1], [hs[b]] if len(hs[b]) else None, noise=v[b:b + 1], snr=snr[b:b + 1], E=800, peak=0.99)
        assert np.array_equal(alone[0][0], noisy[b]) and np.array_equal(alone[1][0], tgt[b]), b
    # a batch without any RIR array at all: unit convolution for every row
    n2, t2 = run(x, None, E=800, peak=0.0)
    assert np.array_equal(n2, x) and np.array_equal(t2, x)


def test_snr_mixing():
    B, Ln = 4, 8000
    x = _signals(B, Ln, seed=7)
    v = (0.05 * np.random.default_rng(8).standard_normal((B, Ln))).astype(np.float32)
    hs = [_rir(40 + b, 2000) for b in range(B)]
    snr = [-5.0, 0.0, 20.0, 40.0]
    noisy, tgt = run(x, hs, noise=v, snr=snr, E=0, peak=0.0)
    ref_noisy, ref_tgt, rows = rr.reverb_mix(x, v, hs, E=0, snr_db=snr, peak=0.0)
    for b in range(B):
        got = rr.snr_of(rows[b]["wet"], noisy[b])
        _log("reverb snr request %.1f dB: float64 SNR of the output %.6f dB" % (snr[b], got))
        assert abs(got - snr[b]) < 1e-3
        bound = _bound(x[b], hs[b])
        assert float(rr.rel_err(noisy[b], ref_noisy[b])[0]) <= bound
        assert np.array_equal(tgt[b], x[b])
    # with the guard and an early target: the pair against the reference
    noisy, tgt = run(x, hs, noise=v, snr=snr, E=800, peak=0.99)
    ref_noisy, ref_tgt, rows = rr.reverb_mix(x, v, hs, E=800, snr_db=snr, peak=0.99)
    for b in range(B):
        assert float(rr.rel_err(noisy[b], ref_noisy[b])[0]) <= _bound(x[b], hs[b])
        assert float(rr.rel_err(tgt[b], ref_tgt[b])[0]) <= _bound(x[b], hs[b][:800])
    # silent noise, silent speech: g = 1, finite
    x2, v2 = x.copy(), v.copy()
    v2[1] = 0.0
    x2[2] = 0.0
    noisy, tgt = run(x2, hs, noise=v2, snr=snr, E=0, peak=0.99)
    ref_noisy, ref_tgt, rows = rr.reverb_mix(x2, v2, hs, E=0, snr_db=snr, peak=0.99)
    assert np.isfinite(noisy).all() and np.isfinite(tgt).all()
    assert rows[1]["g"] == 1.0 and rows[2]["g"] == 1.0
    assert float(rr.rel_err(noisy[1], ref_noisy[1])[0]) <= _bound(x2[1], hs[1])
    assert np.array_equal(noisy[2], v2[2])                               # silent speech: wet = 0 exactly, noisy = 1 * v
    assert np.array_equal(tgt[2], x2[2])
    # snr without noise, noise without snr: unit gain
    n3, _ = run(x, hs, noise=v, snr=None, E=0, peak=0.0)
    r3, _, _ = rr.reverb_mix(x, v, hs, E=0, snr_db=None, peak=0.0)
    assert all(float(rr.rel_err(n3[b], r3[b])[0]) <= _bound(x[b], hs[b]) for b in range(B))


def test_peak_guard():
    B, Ln = 3, 4000
    x = _signals(B, Ln, seed=9)
    x[1] *= 4.0                                                          # 0.4 randn: this row clips
    v = (0.05 * np.random.default_rng(10).standard_normal((B, Ln))).astype(np.float32)
    hs = [_rir(50 + b, 1500) for b in range(B)]
    noisy, tgt = run(x, hs, noise=v, E=800, peak=0.99)
    ref_noisy, ref_tgt, rows = rr.reverb_mix(x, v, hs, E=800, peak=0.99)
    free, tfree = run(x, hs, noise=v, E=800, peak=0.0)                   # peak <= 0: nothing is rescaled
    ref_free, ref_tfree, rows_free = rr.reverb_mix(x, v, hs, E=800, peak=0.0)
    assert rows[1]["scale"] < 1.0 and rows[0]["scale"] == 1.0 and rows[2]["scale"] == 1.0
    assert all(r["scale"] == 1.0 for r in rows_free)
    assert np.max(np.abs(free[1])) > 0.99
    assert np.max(np.abs(noisy[1])) <= 0.99 * (1 + 1e-6)
    for b in range(B):
        assert float(rr.rel_err(noisy[b], ref_noisy[b])[0]) <= _bound(x[b], hs[b])
        assert float(rr.rel_err(tgt[b], ref_tgt[b])[0]) <= _bound(x[b], hs[b][:800])     # the same factor as the reference's
        assert float(rr.rel_err(free[b], ref_free[b])[0]) <= _bound(x[b], hs[b])
        assert float(rr.rel_err(tfree[b], ref_tfree[b])[0]) <= _bound(x[b], hs[b][:800])
    for b in (0, 2):                                                     # the other rows are untouched
        assert np.array_equal(noisy[b], free[b]) and np.array_equal(tgt[b], tfree[b])
    neg, tneg = run(x, hs, noise=v, E=800, peak=-1.0)
    assert np.array_equal(neg, free) and np.array_equal(tneg, tfree)
    # the factor on the target is the factor on noisy
    s = float(np.max(np.abs(noisy[1])) / np.max(np.abs(free[1])))
    np.testing.assert_allclose(tgt[1], tfree[1] * np.float32(s), rtol=3e-7, atol=0)


def test_repeatable_bit_for_bit():
    B, Ln = 5, 32000
    x = _signals(B, Ln, seed=11)
    v = 0.5 * _signals(B, Ln, seed=12)
    hs = [_rir(60 + i, k) for i, k in enumerate((300, 1500, 4097, 8000, 12000))]
    a = run(x, hs, noise=v, snr=[0.0, 5.0, 10.0, 15.0, 20.0], E=800, peak=0.5)
    b = run(x, hs, noise=v, snr=[0.0, 5.0, 10.0, 15.0, 20.0], E=800, peak=0.5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.max(np.abs(a[0])) <= 0.5 * (1 + 1e-6)


def _write_wav(path, x):
    from scipy.io import wavfile
    wavfile.write(str(path), SR, np.round(np.clip(x, -1, 1) * 32767).astype(np.int16))


def _check_staged(loader, n_items, seed):
    """one batch built by hand under fixed seeds, pushed through _stage, against reverb_ref on the drawn parameters"""
    random.seed(seed)
    np.random.seed(seed)
    items = [loader.dataset[i] for i in range(n_items)]
    batch = ds._collate_pairs(items)
    side = torch.cuda.Stream()
    target, noisy, fileid, ev = loader._stage(batch, side)
    ev.synchronize()
    B, Ln = len(items), items[0][0].shape[-1]
    assert target.shape == (B, 1, Ln) and noisy.shape == (B, 1, Ln) and target.is_cuda and noisy.is_cuda
    assert fileid == [it[2] for it in items]
    clean = np.stack([it[0][0].numpy() for it in items])
    par = torch.stack([it[3] for it in items])
    aug = ds.DataAugment()(torch.stack([it[1] for it in items]).cuda(), par.numpy()).cpu().numpy()[:, 0]
    rirs = [it[4].numpy() for it in items]
    snr = [it[5] for it in items]
    rv = loader.dataset.reverb
    ref_noisy, ref_tgt, rows = rr.reverb_mix(clean, aug, rirs, E=rv.early_taps, snr_db=snr, peak=0.99)
    got_n, got_t = noisy.cpu().numpy()[:, 0], target.cpu().numpy()[:, 0]
    dry = 5 * 2.0 ** -24          # a row without a convolution: five fp32 roundings (g, g v, the sum, peak / m, the rescale)
    for b in range(B):
        bn = _bound(clean[b], rirs[b]) if len(rirs[b]) else dry
        bt = _bound(clean[b], rirs[b][:rv.early_taps]) if len(rirs[b]) and rv.early_taps else dry
        assert float(rr.rel_err(got_n[b], ref_noisy[b])[0]) <= bn, b
        assert float(rr.rel_err(got_t[b], ref_tgt[b])[0]) <= bt, b
    return rirs


def test_loader_reverberates_from_rir_files(tmp_path):
    g = np.random.default_rng(13)
    crop = SR // 4
    for d in ("clean", "keyboard", "rir"):
        os.makedirs(str(tmp_path / d))
    for i in range(4):
        _write_wav(tmp_path / "clean" / ("fileid_%d.wav" % i), 0.1 * g.standard_normal(crop + 500 + 37 * i))
    for i in range(2):
        _write_wav(tmp_path / "keyboard" / ("n%d.wav" % i), 0.1 * g.standard_normal(crop))
    for i, delay in enumerate((0, 40, 333)):                             # two of the three start with a delay
        h = np.zeros(delay + 1500)
        h[delay] = 0.8
        h[delay + 1:] = 0.1 * g.standard_normal(1499) * np.exp(-np.arange(1499) / 300.0)
        _write_wav(tmp_path / "rir" / ("r%d.wav" % i), h)
    rv = ds.Reverb(rir_root=str(tmp_path / "rir"), sample_rate=SR, p_reverb=0.75, target="early")
    loader = ds.load_CleanNoisyPairDataset(str(tmp_path), "training", 0.25, 2, SR, num_workers=0, reverb=rv, snr_db=(0, 20))
    random.seed(1)
    np.random.seed(1)
    seen = 0
    for target, noisy, fileid in loader:
        assert target.is_cuda and noisy.is_cuda and target.shape == noisy.shape == (len(fileid), 1, crop)
        assert torch.isfinite(target).all() and torch.isfinite(noisy).all()
        seen += len(fileid)
    assert seen == 4
    rirs = _check_staged(loader, 4, seed=2)
    assert any(len(h) for h in rirs)
    assert all(h[0] == 1.0 and len(h) <= 1500 for h in rirs if len(h))   # prepare(): direct path first, normalised


def test_loader_reverberates_synthetic_items():
    loader = ds.load_CleanNoisyPairDataset("synthetic:8", "training", 0.5, 4, SR, num_workers=0, reverb=ds.Reverb(),
                                           snr_db=(0, 20))
    random.seed(4)
    np.random.seed(4)
    n = 0
    for target, noisy, fileid in loader:
        assert target.is_cuda and target.shape == noisy.shape == (4, 1, SR // 2)
        assert torch.isfinite(noisy).all() and float(noisy.abs().max()) <= 0.99 * (1 + 1e-6)
        n += 1
    assert n == 2
    _check_staged(loader, 4, seed=5)
    # snr_db alone: no room, the clean signal is the target and the noise sits at the requested level
    only = ds.load_CleanNoisyPairDataset("synthetic:4", "training", 0.5, 4, SR, num_workers=0, snr_db=(10, 10))
    target, noisy, fileid = next(iter(only))
    t, n = target.double().cpu().numpy()[:, 0], noisy.double().cpu().numpy()[:, 0]
    assert np.max(np.abs(n)) < 0.99                                      # no rescale in this batch
    for b in range(4):
        assert abs(rr.snr_of(t[b], n[b]) - 10.0) < 1e-3
    # the plain loader is what it was: (clean, noisy, fileid), noisy = clean + augmented noise
    plain = ds.load_CleanNoisyPairDataset("synthetic:4", "training", 0.5, 4, SR, num_workers=0)
    clean, noisy, fileid = next(iter(plain))
    assert clean.shape == noisy.shape == (4, 1, SR // 2) and len(fileid) == 4
