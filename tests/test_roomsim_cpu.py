"""CPU: the room simulator's float64 restatement against closed forms, the host side of RoomSim (draws, rows, argument
checks), the entry point's refusals and the generator's integer part."""
import math
import os
import pickle
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roomsim_ref as rr  # noqa: E402
from tinyrecurrentunet_amd import _lib  # noqa: E402
from tinyrecurrentunet_amd import dataset as ds  # noqa: E402

FS, C, TW = 16000, 343.0, 81


def _row(dim, src, mic, beta, rt60=0.5, seed=1):
    return ds.RoomSim.row(dim, src, mic, beta, rt60, seed).numpy()


def _tap_train(tau, gain, n_taps, tw=TW):
    """one image by the formula of the issue, tap by tap in Python floats"""
    h = np.zeros(n_taps)
    for n in range(n_taps):
        t = n - tau
        if abs(t) < tw / 2.0:
            sinc = 1.0 if t == 0 else (0.0 if t == round(t) else math.sin(math.pi * t) / (math.pi * t))
            h[n] += gain * 0.5 * (1.0 + math.cos(2.0 * math.pi * t / tw)) * sinc
    return h


def test_no_reflection_is_exactly_a_unit_tap():
    for dim, s, r in (((5, 4, 3), (1, 1, 1), (2, 2, 1.5)), ((2.5, 3.1, 2.2), (0.9, 1.2, 1.0), (1.7, 2.0, 1.4))):
        h, n_img = rr.ism(_row(dim, s, r, 0.0), 800, FS)
        want = np.zeros(800)
        want[0] = 1.0
        assert np.array_equal(h, want)
        assert n_img >= 1


def test_one_reflective_wall_is_two_images_with_hand_computed_gain_and_delay():
    dim, s, r = (5.0, 4.0, 3.0), (1.0, 1.5, 1.25), (2.5, 2.0, 1.5)     # every number exact in float32, like the row
    d0 = math.sqrt(1.5 ** 2 + 0.5 ** 2 + 0.25 ** 2)
    # the wall at x = 0: the image sits at x = -sx
    d1 = math.sqrt((-1.0 - 2.5) ** 2 + 0.5 ** 2 + 0.25 ** 2)
    h, _ = rr.ism(_row(dim, s, r, (0.75, 0, 0, 0, 0, 0)), 400, FS)
    want = _tap_train(0.0, 1.0, 400) + _tap_train((d1 - d0) * FS / C, 0.75 * d0 / d1, 400)
    np.testing.assert_allclose(h, want, rtol=0, atol=1e-14)
    # the wall at x = Lx: the image sits at x = 2 Lx - sx; with the coefficients swapped it is the only reflection
    d2 = math.sqrt((2 * 5.0 - 1.0 - 2.5) ** 2 + 0.5 ** 2 + 0.25 ** 2)
    h, _ = rr.ism(_row(dim, s, r, (0, 0.625, 0, 0, 0, 0)), 400, FS)
    want = _tap_train(0.0, 1.0, 400) + _tap_train((d2 - d0) * FS / C, 0.625 * d0 / d2, 400)
    np.testing.assert_allclose(h, want, rtol=0, atol=1e-14)
    # a short delay: the pre-ringing of the reflection falls on negative taps and is dropped, not wrapped
    s2 = (0.0625, 1.5, 1.25)
    d0 = math.sqrt(2.4375 ** 2 + 0.5 ** 2 + 0.25 ** 2)
    d1 = math.sqrt(2.5625 ** 2 + 0.5 ** 2 + 0.25 ** 2)
    tau = (d1 - d0) * FS / C
    assert tau < TW / 2.0
    h, _ = rr.ism(_row(dim, s2, r, (0.75, 0, 0, 0, 0, 0)), 400, FS)
    np.testing.assert_allclose(h, _tap_train(0.0, 1.0, 400) + _tap_train(tau, 0.75 * d0 / d1, 400), rtol=0, atol=1e-14)
    assert np.all(h[int(tau) + 42:] == 0.0)


def test_gain_exponents_follow_the_wall_convention():
    """six distinct coefficients, source off-centre on every axis, against a plain triple loop over the lattice"""
    fs, n_taps = 8000, 160
    row = _row((3.0, 2.6, 2.2), (0.7, 1.9, 0.6), (2.1, 0.8, 1.5), (0.5, 0.9, 0.6, 0.85, 0.7, 0.8))
    v = row.astype(np.float64)                              # the row's float32 values are the exact inputs
    dim, s, r, beta = tuple(v[0:3]), tuple(v[3:6]), tuple(v[6:9]), tuple(v[9:15])
    assert len(set(beta)) == 6 and all(abs(s[a] - dim[a] / 2) > 0.2 for a in range(3))
    d0 = math.dist(s, r)
    want = np.zeros(n_taps)
    N = 4                                                   # (160 + 41) taps are 8.6 m: orders up to 2 on the 2.2 m axis
    for mx in range(-N, N + 1):
        for my in range(-N, N + 1):
            for mz in range(-N, N + 1):
                for q in (0, 1):
                    for j in (0, 1):
                        for k in (0, 1):
                            img = ((1 - 2 * q) * s[0] + 2 * mx * dim[0], (1 - 2 * j) * s[1] + 2 * my * dim[1],
                                   (1 - 2 * k) * s[2] + 2 * mz * dim[2])
                            d = math.dist(img, r)
                            tau = (d - d0) * fs / C
                            if tau - TW / 2.0 >= n_taps:
                                continue
                            gain = (beta[0] ** abs(mx - q) * beta[1] ** abs(mx) * beta[2] ** abs(my - j) * beta[3] ** abs(my)
                                    * beta[4] ** abs(mz - k) * beta[5] ** abs(mz)) * d0 / d
                            want += _tap_train(tau, gain, n_taps)
    h, _ = rr.ism(row, n_taps, fs)
    np.testing.assert_allclose(h, want, rtol=0, atol=1e-12)
    # one image by hand: q = 1, mx = 1 (once off the wall at x = Lx); j = 0, my = -1 (off both y walls); k = 1, mz = 0 (z0)
    img = (-s[0] + 2 * dim[0], s[1] - 2 * dim[1], -s[2])
    d = math.dist(img, r)
    gain = beta[1] * beta[2] * beta[3] * beta[4] * d0 / d
    dd, gg = rr.images(row, d + 1.0)
    i = int(np.argmin(np.abs(dd - d)))
    assert abs(dd[i] - d) < 1e-12 and abs(gg[i] * d0 / dd[i] - gain) < 1e-15


def test_hybrid_row_layout_and_length():
    row = _row((5, 4, 3), (1, 1, 1), (2, 2, 1.5), 0.8, rt60=0.2, seed=77)
    o = rr.rir(row, fs=FS, ism_ms=50.0, max_rir_sec=0.25)
    assert (o["n_c"], o["K"], o["n_ism"], len(o["h"])) == (800, 3200, 800, 4000)
    assert o["h"][0] == 1.0 and np.all(o["h"][3200:] == 0.0) and o["sigma"] > 0
    n = np.arange(800, 3200)
    np.testing.assert_allclose(o["env"][800:3200], o["sigma"] * np.exp(-6.9078 * (n - 800 + 80) / (0.2 * FS)), rtol=1e-6)
    np.testing.assert_allclose(o["h"][800:3200], o["env"][800:3200] * rr.normal(77, n), rtol=1e-12)
    assert o["sigma"] == pytest.approx(math.sqrt(np.mean(o["h"][640:800] ** 2)))
    short = rr.rir(_row((5, 4, 3), (1, 1, 1), (2, 2, 1.5), 0.8, rt60=0.03), fs=FS, ism_ms=50.0, max_rir_sec=0.25)
    assert (short["K"], short["n_ism"], short["sigma"]) == (480, 480, 0.0) and np.all(short["h"][480:] == 0.0)
    for bad in (np.zeros(18), np.full(18, np.nan), _row((0.01, 0.01, 0.01), (0.005,) * 3, (0.006,) * 3, 0.5)):
        o = rr.rir(bad, fs=FS, ism_ms=50.0, max_rir_sec=0.25)
        assert o["K"] == 0 and not np.any(o["h"])


def test_generator_integer_part_by_hand():
    """lowbias32 and the two words of a tap, against values worked out with plain Python integers"""
    assert [int(x) for x in rr.mix([0, 1, 0xFFFFFFFF, 0x12345678])] == [0x0, 0x688990c0, 0x6768824a, 0xf5e71c96]
    for seed, n, a, b in ((0, 0, 0x944fb554, 0xc67c684d), (1, 0, 0x603c7207, 0x747b0d1a), (1, 1, 0x68e97049, 0x5225b6bc),
                          (0xDEADBEEF, 65535, 0x83abfbb1, 0x82e80e2e), (0xFFFFFFFF, 12345, 0xd110d1d5, 0xf91a492f)):
        wa, wb = rr.words(seed, [n])
        assert (int(wa[0]), int(wb[0])) == (a, b)
    # seed 1, tap 0: u1 = (0x603c72 + 1) / 2^24, u2 = 0x747b0d / 2^24
    g = math.sqrt(-2.0 * math.log((0x603c72 + 1) / 2.0 ** 24)) * math.cos(2.0 * math.pi * 0x747b0d / 2.0 ** 24)
    assert rr.normal(1, [0])[0] == pytest.approx(g, rel=1e-14)
    x = rr.normal(7, np.arange(200000))
    assert abs(x.mean()) < 0.01 and abs(x.std() - 1.0) < 0.01       # 4 sigma of 200000 normal samples is 0.009
    assert abs(np.corrcoef(x[:-1], x[1:])[0, 1]) < 0.01
    assert abs(np.corrcoef(x[:65536], rr.normal(8, np.arange(65536)))[0, 1]) < 0.016


def test_draw_keeps_the_margins_and_is_repeatable():
    sim = ds.RoomSim()
    random.seed(5)
    rows = [sim.draw() for _ in range(1000)]
    again_state = random.getstate()
    for row in rows:
        assert row.dtype == torch.float32 and row.shape == (ds.RoomSim.ROW,)
        f = ds.RoomSim.fields(row)
        for (lo, hi), v, s, r in zip(sim.room_dim, f["dim"], f["src"], f["mic"]):
            assert np.float32(lo) <= v <= np.float32(hi)
            assert 0.5 <= s <= v - 0.5 and 0.5 <= r <= v - 0.5
        assert 0.3 <= math.dist(f["src"], f["mic"]) <= 3.0
        assert np.float32(0.2) <= f["rt60"] <= np.float32(1.0)
        assert len(set(f["beta"])) == 1
        assert f["beta"][0] == pytest.approx(rr.sabine(f["dim"], f["rt60"]), rel=1e-6)
        assert rr.valid(row.numpy())
        # the seed travels as two exactly representable 16-bit halves
        lo16, hi16 = float(row[16]), float(row[17])
        assert lo16 == int(lo16) and hi16 == int(hi16) and 0 <= lo16 < 65536 and 0 <= hi16 < 65536
        assert f["seed"] == int(lo16) + 65536 * int(hi16)
        assert torch.equal(ds.RoomSim.row(**f), row)            # the round trip
    assert len({ds.RoomSim.fields(r)["seed"] for r in rows}) > 990
    random.seed(5)
    assert all(torch.equal(a, sim.draw()) for a in rows)
    assert random.getstate() == again_state
    # explicit rows
    row = ds.RoomSim.row((5, 4, 3), (1, 1, 1), (2, 2, 1.5), 0.75, 0.4, 0xFFFF0001)
    assert row[9:15].tolist() == [0.75] * 6 and row[16:].tolist() == [1.0, 65535.0]
    assert ds.RoomSim.fields(row)["seed"] == 0xFFFF0001
    with pytest.raises(ValueError):
        ds.RoomSim.row((5, 4, 3), (1, 1, 1), (2, 2, 1.5), (0.5, 0.5), 0.4, 1)
    with pytest.raises(ValueError):
        ds.RoomSim.row((5, 4, 3), (1, 1, 1), (2, 2, 1.5), 0.5, 0.4, 2 ** 32)
    # Sabine: alpha = 0.161 V / (S rt60), clipped at 0.99
    assert ds.RoomSim.sabine((5, 4, 3), 0.5) == pytest.approx(math.sqrt(1 - 0.161 * 60 / (94 * 0.5)))
    assert ds.RoomSim.sabine((10, 8, 4), 0.01) == pytest.approx(math.sqrt(0.01))
    # parameters only: the object pickles for the DataLoader workers
    sim._ws["x"] = object()
    clone = pickle.loads(pickle.dumps(ds.Reverb(room=sim, target="early")))
    assert clone.room._ws == {} and clone.room.n_c == 1280 and clone.room.max_taps == 16000


def test_roomsim_and_reverb_argument_errors(tmp_path):
    for kw in (dict(room_dim=((1.9, 5), (3, 8), (2.4, 4))), dict(room_dim=((3, 10), (3, 8))), dict(room_dim=((5, 4), (3, 8), (3, 4))),
               dict(ism_ms=600.0), dict(ism_ms=0.0), dict(tw=80), dict(tw=131), dict(max_rir_sec=5.0), dict(wall_margin=1.3),
               dict(distance=(9.0, 10.0)), dict(distance=(0.0, 3.0)), dict(rt60=(0.0, 1.0)), dict(sample_rate=2000, ism_ms=2200.0),
               dict(room_dim=((2, 400), (2, 400), (2, 400)), ism_ms=500.0)):
        with pytest.raises(ValueError):
            ds.RoomSim(**kw)
    assert ds.RoomSim(ism_ms=512.0).n_c == 8192                 # the cap itself is accepted
    assert ds.RoomSim(sample_rate=48000).n_c == 3840 and ds.RoomSim(sample_rate=48000).max_taps == 48000
    from scipy.io import wavfile
    wavfile.write(str(tmp_path / "a.wav"), 16000, np.array([30000, 1000], dtype=np.int16))
    with pytest.raises(ValueError):
        ds.Reverb(rir_root=str(tmp_path), room=ds.RoomSim())
    with pytest.raises(ValueError):
        ds.Reverb(sample_rate=16000, room=ds.RoomSim(sample_rate=48000))
    with pytest.raises(ValueError):
        ds.Reverb(room=ds.RoomSim(ism_ms=40.0), target="early", early_ms=50.0)
    assert ds.Reverb(room=ds.RoomSim(ism_ms=40.0), target="dry", early_ms=50.0).early_taps == 0
    assert ds.Reverb(room=ds.RoomSim(ism_ms=50.0), target="early", early_ms=50.0).early_taps == 800
    # room mode draws a parameter row or nothing, repeatably
    rv = ds.Reverb(room=ds.RoomSim(), p_reverb=0.5)
    random.seed(9)
    got = [rv.draw() for _ in range(40)]
    assert all(h.dtype == torch.float32 and h.numel() in (0, ds.RoomSim.ROW) for h in got)
    assert 5 < sum(h.numel() == 0 for h in got) < 35
    random.seed(9)
    assert all(torch.equal(a, rv.draw()) for a in got)
    # the dataset carries the rows like taps and the collate pads absent rooms with zeros
    random.seed(1)
    np.random.seed(2)
    d = ds.CleanNoisyPairDataset("synthetic:4", "training", 0.25, 16000, reverb=rv, snr_db=(0.0, 20.0))
    batch = ds._collate_pairs([d[i] for i in range(4)])
    assert batch[4].shape[1] in (0, ds.RoomSim.ROW) and set(batch[5].tolist()) <= {0, ds.RoomSim.ROW}
    for b in range(4):
        assert (batch[5][b] == 0) == (not bool(batch[4][b].any()))
    import dropin.dataset as shim
    assert shim.RoomSim is ds.RoomSim


def test_rir_ism_refuses_before_any_launch():
    lib = _lib.lib()
    EINVAL, ENOTSUP = _lib.TRUNET_EINVAL, _lib.TRUNET_ENOTSUP
    need = lib.trunet_rir_ism_workspace_bytes(4, 16000)
    assert need > 0
    assert lib.trunet_rir_ism_workspace_bytes(0, 16000) == 0 and lib.trunet_rir_ism_workspace_bytes(4, 0) == 0
    assert lib.trunet_rir_ism_workspace_bytes(4, 65537) == 0 and lib.trunet_rir_ism_workspace_bytes(4, 65536) > 0
    rooms, rir, lens, ws = (0x10000000 * (i + 1) for i in range(4))

    def call(rooms=rooms, row=18, rir=rir, lens=lens, B=4, K=16000, fs=16000.0, c=343.0, n_c=1280, tw=81, mx=1.0, ws=ws,
             ws_bytes=need):
        return lib.trunet_rir_ism(rooms, row, rir, lens, B, K, fs, c, n_c, tw, mx, ws, ws_bytes, None)
    assert call(rooms=None) == EINVAL and call(rir=None) == EINVAL and call(lens=None) == EINVAL and call(ws=None) == EINVAL
    assert call(row=17) == EINVAL and call(row=19) == EINVAL and call(row=0) == EINVAL
    assert call(B=0) == EINVAL and call(B=-1) == EINVAL and call(B=65536) == EINVAL and call(K=0) == EINVAL
    assert call(n_c=0) == EINVAL and call(tw=0) == EINVAL and call(tw=-3) == EINVAL
    assert call(fs=0.0) == EINVAL and call(fs=float("nan")) == EINVAL and call(fs=float("inf")) == EINVAL
    assert call(c=0.0) == EINVAL and call(c=-343.0) == EINVAL and call(mx=0.0) == EINVAL and call(mx=float("nan")) == EINVAL
    assert call(ws_bytes=need - 1) == EINVAL
    assert call(K=65537) == ENOTSUP and call(n_c=8193) == ENOTSUP
    assert call(tw=80) == ENOTSUP and call(tw=131) == ENOTSUP and call(tw=2) == ENOTSUP
    assert call(fs=4000.0, n_c=8192) == ENOTSUP                     # 8192 taps at 4 kHz are 700 m of images
    assert call(c=3430.0, n_c=8192) == ENOTSUP


def test_restatement_decay_and_tail_energy():
    """Two properties of the restatement alone, not bars for the kernel.  A 5 x 4 x 3 m room drawn by
    RoomSim with Sabine's coefficient: (1) the Schroeder decay (T20 fit) of the image-source part alone, with ism_ms at the
    cap, against the requested rt60; (2) the energy of the tail's first W taps against the last W image-source taps.
    Over 20 seeded rooms (rt60 in [0.25, 0.6] s) the restatement itself gave RT60 ratios of 1.24 to 1.43 and energy
    steps of -2.7 to -0.1 dB; the assertions below are those ranges widened by their own width.  The image-source decay is
    slower than requested because Sabine's formula overstates the decay of a room this absorbent (Eyring's would be closer);
    the step is the tail's envelope running W taps later than the window sigma_c is taken from: -0.6 dB / rt60."""
    random.seed(2024)
    row = ds.RoomSim(room_dim=((5, 5), (4, 4), (3, 3)), rt60=(0.25, 0.6)).draw().numpy()
    h, _ = rr.ism(row, 8192, FS)
    ratio = rr.schroeder_rt60(h, FS) / float(row[15])
    o = rr.rir(row, fs=FS, ism_ms=80.0, max_rir_sec=1.0)
    step_db = 10.0 * math.log10(np.sum(o["h"][1280:1440] ** 2) / np.sum(o["h"][1120:1280] ** 2))
    print("schroeder rt60 / requested %.3f, tail energy step %.2f dB" % (ratio, step_db))
    assert 1.05 < ratio < 1.62
    assert -5.3 < step_db < 2.5
