"""GPU: the room simulator (roomsim.hip, dataset.RoomSim, Reverb(room=...)) against its float64 statement
(tests/roomsim_ref.py), the only yardstick there is.

Bars.  Image-source taps: max|got - ref| / max|ref| per row (max|ref| = 1, the direct path).  Tail taps: max|got - ref| in
units of the envelope sigma_c exp(.) of that tap.  Worst figures measured over the cases of this file on an MI355X:
    image-source part  4.014e-08  (the small room at 48 kHz; 2.4e-08 to 3.7e-08 on the other rows, 1.7e5 images included)
    tail               8.384e-07  (the rt60 = 0.2 s row of the ragged batch; 4.6e-07 to 8.2e-07 on the other rows)
The bars are 4x those: ISM_BAR and TAIL_BAR below.  Whatever is measured, the image-source bar stays below 1e-4: with fp64
delays a tap is a sum of at most a few hundred fp32 terms, and a larger error means wrong delay arithmetic or a wrong lane
map."""
import functools
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roomsim_ref as rr  # noqa: E402
from tinyrecurrentunet_amd import _lib  # noqa: E402
from tinyrecurrentunet_amd import dataset as ds  # noqa: E402

pytestmark = pytest.mark.gpu

ISM_BAR = 1.61e-7
TAIL_BAR = 3.36e-6
assert ISM_BAR < 1e-4

SMALL = dict(dim=(2.5, 3.1, 2.2), src=(0.9, 1.2, 1.0), mic=(1.7, 2.0, 1.4), beta=(0.5, 0.9, 0.6, 0.8, 0.7, 0.85))
LIVING = dict(dim=(5.0, 4.0, 3.0), src=(1.0, 1.5, 1.25), mic=(2.5, 2.0, 1.5))


def _log(msg):
    """print a measured figure; with TRUNET_PARITY_DIR set to a folder, also append it to parity_roomsim.txt there"""
    print(msg)
    out_dir = os.environ.get("TRUNET_PARITY_DIR")
    if out_dir and os.path.isdir(out_dir):
        open(os.path.join(out_dir, "parity_roomsim.txt"), "a").write(msg + "\n")


def _small(rt60=0.25, seed=12345):
    return ds.RoomSim.row(rt60=rt60, seed=seed, **SMALL).numpy()


def _hybrid(rt60, seed):
    return ds.RoomSim.row(beta=rr.sabine(LIVING["dim"], 0.4), rt60=rt60, seed=seed, **LIVING).numpy()


def _ragged():
    """the rows of cases 3 and 4 (four of them: one room, three rt60), a row of zeros, a row of NaN and a 1 cm room"""
    tiny = ds.RoomSim.row((0.01, 0.01, 0.01), (0.004,) * 3, (0.006,) * 3, 0.5, 0.3, 5).numpy()
    return np.stack([_small(), _hybrid(0.03, 1), _hybrid(0.2, 2), _hybrid(0.6, 3), np.zeros(18, np.float32),
                     np.full(18, np.nan, np.float32), tiny])


def run(rows, fs=16000, ism_ms=50.0, max_rir_sec=0.25, kmax=None, tw=81, c=343.0):
    """trunet_rir_ism on numpy rows -> (rir (B, Kmax), lens (B,)) as numpy; the output is prefilled with NaN"""
    lib = _lib.lib()
    dev = torch.device("cuda")
    rows = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.float32)
    B = rows.shape[0]
    K = int(round(max_rir_sec * fs)) if kmax is None else kmax
    r = torch.from_numpy(rows).to(dev)
    out = torch.full((B, K), float("nan"), device=dev, dtype=torch.float32)
    lens = torch.full((B,), -7, device=dev, dtype=torch.int32)
    nbytes = int(lib.trunet_rir_ism_workspace_bytes(B, K))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = lib.trunet_rir_ism(r.data_ptr(), 18, out.data_ptr(), lens.data_ptr(), B, K, float(fs), float(c),
                            int(round(ism_ms * fs / 1000.0)), tw, float(max_rir_sec), ws.data_ptr(), nbytes,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy(), lens.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ref(row_bytes, fs, ism_ms, max_rir_sec):
    """the restatement of one row, computed once and shared (treat the result as read-only)"""
    return rr.rir(np.frombuffer(row_bytes, dtype=np.float32), fs=fs, ism_ms=ism_ms, max_rir_sec=max_rir_sec)


def _check(tag, got, glen, row, fs, ism_ms, max_rir_sec):
    """one row against the restatement: length, image-source part, tail (in envelope units), zeros beyond K_b"""
    o = _ref(np.asarray(row, np.float32).tobytes(), fs, ism_ms, max_rir_sec)
    K, n_ism, n_c = o["K"], o["n_ism"], o["n_c"]
    assert glen == K, (tag, glen, K)
    assert not np.any(np.isnan(got))
    assert np.all(got[K:] == 0.0), tag
    e_ism = e_tail = 0.0
    if n_ism:
        e_ism = float(np.max(np.abs(got[:n_ism] - o["h"][:n_ism])) / np.max(np.abs(o["h"][:n_ism])))
    if K > n_c:
        e_tail = float(np.max(np.abs(got[n_c:K] - o["h"][n_c:K]) / o["env"][n_c:K]))
    _log("roomsim %-28s K %5d n_ism %5d images %7d  ism err %.3e  tail err %.3e" % (tag, K, n_ism, o["images"], e_ism, e_tail))
    assert e_ism <= ISM_BAR, (tag, e_ism)
    assert e_tail <= TAIL_BAR, (tag, e_tail)
    return o


@pytest.mark.parametrize("kmax", [1, 40, 511, 512, 513, 1023, 1024, 1025, 2049])
def test_no_reflection_is_a_unit_tap_bit_for_bit(kmax):
    """beta = 0: h[0] == 1.0 and every other tap 0.0, for a segment of one tap, a window cut at tap 0 and both sides of
    the edges of the 512-tap segments"""
    rows = np.stack([ds.RoomSim.row(beta=0.0, rt60=1.0, seed=3, **LIVING).numpy(),
                     ds.RoomSim.row(rt60=1.0, seed=4, **{**SMALL, "beta": 0.0}).numpy()])
    got, lens = run(rows, ism_ms=250.0, max_rir_sec=1.0, kmax=kmax)
    want = np.zeros((2, kmax), np.float32)
    want[:, 0] = 1.0
    assert lens.tolist() == [kmax, kmax]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_one_reflective_wall():
    """two images; the reflection arrives within tw / 2 of the direct path, so its pre-ringing falls on negative taps"""
    row = ds.RoomSim.row((5.0, 4.0, 3.0), (0.0625, 1.5, 1.25), (2.5, 2.0, 1.5), (0.75, 0, 0, 0, 0, 0), 0.25, 9).numpy()
    got, lens = run(row, ism_ms=250.0)
    o = _check("one wall", got[0], lens[0], row, 16000, 250.0, 0.25)
    assert o["images"] == 2
    tau = (np.sqrt(2.5625 ** 2 + 0.3125) - np.sqrt(2.4375 ** 2 + 0.3125)) * 16000 / 343.0
    assert tau < 40.5 and np.all(got[0, int(tau) + 42:] == 0.0)             # dropped, not wrapped to the end of the row


@pytest.mark.parametrize("fs,ism_ms", [(16000, 250.0), (48000, 80.0)])
def test_full_small_room(fs, ism_ms):
    """2.5 x 3.1 x 2.2 m, six distinct coefficients: about 1.7e5 images at 16 kHz, an image-source-only row; the same room
    at 48 kHz with an 80 ms image-source part and a tail"""
    row = _small()
    got, lens = run(row, fs=fs, ism_ms=ism_ms)
    o = _check("small room %d Hz" % fs, got[0], lens[0], row, fs, ism_ms, 0.25)
    assert (o["K"] > o["n_c"]) == (fs == 48000)


@pytest.mark.parametrize("rt60", [0.03, 0.2, 0.6])
def test_hybrid_rows(rt60):
    row = _hybrid(rt60, 11)
    got, lens = run(row)
    o = _check("hybrid rt60 %.2f" % rt60, got[0], lens[0], row, 16000, 50.0, 0.25)
    assert o["K"] == {0.03: 480, 0.2: 3200, 0.6: 4000}[rt60] and (o["K"] > o["n_c"]) == (rt60 > 0.05)


def test_ragged_batch_and_independence():
    """good, absent and malformed rows in one launch (the issue counts B = 6; its list of rows has seven); then every row
    alone, in a permuted batch, under 2 Kmax and on a second run gives the same bits"""
    rows = _ragged()
    got, lens = run(rows)
    assert not np.any(np.isnan(got))
    assert lens[4:].tolist() == [0, 0, 0] and not np.any(got[4:])
    for b in range(4):
        _check("ragged row %d" % b, got[b], lens[b], rows[b], 16000, 50.0, 0.25)
    bits = got.view(np.uint32)
    again, lens2 = run(rows)
    assert np.array_equal(again.view(np.uint32), bits) and np.array_equal(lens2, lens)
    perm = [5, 3, 0, 6, 2, 4, 1]
    pg, pl = run(rows[perm])
    assert np.array_equal(pg.view(np.uint32), bits[perm]) and np.array_equal(pl, lens[perm])
    wide, wl = run(rows, kmax=8000)
    assert np.array_equal(wide[:, :4000].view(np.uint32), bits) and not np.any(wide[:, 4000:]) and np.array_equal(wl, lens)
    for b in range(len(rows)):
        one, ol = run(rows[b])
        assert np.array_equal(one[0].view(np.uint32), bits[b]) and ol[0] == lens[b]


def _seed_all(n):
    random.seed(n)
    np.random.seed(n)
    torch.manual_seed(n)


def test_loader_route_equals_the_manual_composition():
    """load_CleanNoisyPairDataset with Reverb(room=RoomSim()) against room(rows) followed by a Reverb WITHOUT a room on the
    taps (the existing path), bit for bit; rows drawn without a room are plain pairs"""
    sim = ds.RoomSim()
    rv = ds.Reverb(room=sim, p_reverb=0.5, target="early")
    loader = ds.load_CleanNoisyPairDataset("synthetic:8", "training", 1, 4, 16000, num_workers=0, reverb=rv, snr_db=(0, 20))
    _seed_all(21)
    got = [(t.clone(), n.clone(), ids) for t, n, ids in loader]
    torch.cuda.synchronize()
    _seed_all(21)
    raw = list(loader.loader)
    assert len(got) == len(raw) == 2
    taps = ds.Reverb(p_reverb=0.5, target="early")
    n_room = n_plain = 0
    for (target, noisy, ids), (clean, other, ids2, params, rows, lens, snr) in zip(got, raw):
        assert ids == ids2 and target.shape == noisy.shape == (4, 1, 16000)
        clean_d, aug = clean.cuda(), ds.DataAugment()(other.cuda(), params=params.numpy())
        h = hl = None
        if rows.shape[1]:
            assert rows.shape[1] == ds.RoomSim.ROW
            h, hl = sim(rows.cuda())
            assert h.shape == (4, 16000) and (hl == 0).tolist() == (lens == 0).tolist()
        want_noisy, want_target = taps(clean_d, h, hl, noise=aug, snr_db=snr.cuda())
        assert torch.equal(noisy, want_noisy) and torch.equal(target, want_target)
        assert float(noisy.abs().max()) <= 0.99 * (1 + 1e-6)
        for b, k in enumerate(lens.tolist()):
            peak = float(noisy[b].abs().max())
            if k == 0:                                            # no room: the target is the clean signal (peak-guarded)
                n_plain += 1
                scale = 1.0 if peak < 0.989 else None
                if scale:
                    assert torch.equal(target[b], clean_d[b])
            else:
                n_room += 1
                assert int(hl[b]) >= 3200 and abs(float(h[b, 0]) - 1.0) < 0.05      # the direct path, plus ringing
                assert not torch.equal(target[b], clean_d[b])
    assert n_room > 0 and n_plain > 0
