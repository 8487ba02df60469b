"""Scoring (tinyrecurrentunet_amd/evaluate.py) without a GPU: self-checks of the float64 restatement (tests/metrics_ref.py),
the host-built filter and band tables against it, the resampling closed form against scipy, file pairing, argument errors
and the entry points' host-side checks."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _broadband(n, seed=0):
    return np.random.default_rng(seed).standard_normal(n)


def test_restatement_identity_and_scale_invariance():
    x = _broadband(16000 * 3)
    r = R.stoi_ref(x, x, 16000)
    assert r["segments"] > 0
    assert abs(r["stoi"] - 1) < 1e-9 and abs(r["estoi"] - 1) < 1e-9
    y = x + 0.3 * _broadband(x.shape[0], seed=1)
    base = R.stoi_ref(x, y, 16000)
    for a, b in [(3.0, 1.0), (1.0, 0.25), (0.01, 7.0)]:
        s = R.stoi_ref(a * x, b * y, 16000)
        assert abs(s["stoi"] - base["stoi"]) < 1e-9 and abs(s["estoi"] - base["estoi"]) < 1e-9, (a, b)
        assert s["segments"] == base["segments"]


def test_restatement_stoi_falls_with_the_snr():
    x = _broadband(16000 * 3)
    n = _broadband(x.shape[0], seed=5)
    n *= np.linalg.norm(x) / np.linalg.norm(n)
    vals = [R.stoi_ref(x, x + n * 10 ** (-snr / 20), 16000)["stoi"] for snr in (20, 5, -5)]
    assert vals[0] > vals[1] > vals[2], vals


def test_restatement_si_sdr_of_an_orthogonal_error_is_20_db():
    s = _broadband(20000, seed=2)
    s -= s.mean()
    e = _broadband(20000, seed=3)
    e -= e.mean()
    e -= s * np.dot(e, s) / np.dot(s, s)
    e *= math.sqrt(np.dot(s, s) / 100 / np.dot(e, e))
    assert abs(R.si_sdr_ref(s, s + e) - 20.0) < 1e-9
    assert math.isnan(R.si_sdr_ref(np.zeros(100), np.ones(100)))


def test_restatement_too_short_and_silence():
    x = _broadband(257)
    r = R.stoi_ref(x, x, 16000)
    assert r["stoi"] == 1e-5 and r["estoi"] == 1e-5 and r["segments"] == 0
    # exactly 31 / 30 kept frames at 10 kHz: one segment / too short
    for frames, segs in [(31, 1), (30, 0)]:
        x = _broadband(256 + (frames - 1) * 128 + 1, seed=frames)
        r = R.stoi_ref(x, x + 0.1 * _broadband(x.shape[0], seed=9), 10000)
        assert r["kept"] == frames and r["segments"] == segs, r


def test_host_filter_and_band_table_equal_the_restatement():
    from tinyrecurrentunet_amd import evaluate as E
    for fs, (p, q, taps) in {16000: (5, 8, 581), 48000: (5, 24, 1741), 8000: (5, 4, 365)}.items():
        assert E.ratio(fs) == R.ratio(fs) == (p, q)
        h, half = E.kaiser_filter(p, q)
        hr, Lr = R.kaiser_filter(p, q)
        assert half == Lr and h.shape == (taps,) and np.array_equal(h, hr)
    assert E.ratio(10000) == (1, 1)
    assert np.array_equal(E.band_edges(), R.band_edges())
    assert np.array_equal(E.window(), R.WINDOW)
    for n in (0, 1, 256, 257, 384, 385, 4097, 100000):
        assert E.n_frames(n) == len(range(0, n - 256, 128)), n


@pytest.mark.parametrize("fs", [16000, 48000, 8000])
def test_resampling_closed_form_matches_scipy(fs):
    from scipy.signal import resample_poly
    x = _broadband(12345, seed=fs)
    p, q = R.ratio(fs)
    hn, _ = R.kaiser_filter(p, q)
    y = R.resample(x, fs)
    ref = resample_poly(x, p, q, window=hn)
    assert y.shape == ref.shape == (-(-x.shape[0] * p // q),)
    assert np.max(np.abs(y - ref)) < 1e-12


def test_file_pairing():
    from tinyrecurrentunet_amd.evaluate import pair_files
    clean = ["clean_fileid_0.wav", "clean_fileid_1.wav", "clean_fileid_12.wav", "same.wav", "clean_fileid_5.wav"]
    enh = ["enhanced_fileid_12.wav", "same.wav", "enhanced_fileid_0.wav", "enhanced_fileid_1.wav", "noisy_fileid_99.wav"]
    pairs, unmatched = pair_files(clean, enh)
    assert pairs == [("clean_fileid_0.wav", "enhanced_fileid_0.wav"), ("clean_fileid_1.wav", "enhanced_fileid_1.wav"),
                     ("clean_fileid_12.wav", "enhanced_fileid_12.wav"), ("same.wav", "same.wav")]
    assert unmatched == 2                                   # clean_fileid_5 and noisy_fileid_99
    # an identical name wins over a token; a token shared by two files pairs nothing
    pairs, unmatched = pair_files(["a_fileid_1.wav", "b_fileid_2.wav"],
                                  ["a_fileid_1.wav", "x_fileid_2.wav", "y_fileid_2.wav"])
    assert pairs == [("a_fileid_1.wav", "a_fileid_1.wav")] and unmatched == 3


def test_evaluate_argument_errors_without_a_device():
    from tinyrecurrentunet_amd import _lib
    from tinyrecurrentunet_amd.evaluate import evaluate, validate
    x = [torch.zeros(1000), torch.zeros(500)]
    with pytest.raises(ValueError, match="utterance 1"):
        evaluate(x, [torch.zeros(1000), torch.zeros(499)])
    with pytest.raises(ValueError, match="2 clean and 1"):
        evaluate(x, x[:1])
    with pytest.raises(ValueError, match="pesq"):
        evaluate(x, x, metrics=("stoi", "pesq"))
    with pytest.raises(ValueError, match="44.1 kHz"):
        evaluate(x, x, fs=44100)
    with pytest.raises(ValueError, match="22.05 kHz"):
        evaluate(x, x, fs=22050)
    with pytest.raises(ValueError):
        evaluate(x, x, fs=0)
    with pytest.raises(ValueError, match="lengths"):
        evaluate(torch.zeros(2, 100), torch.zeros(2, 100), lengths=[100, 101])
    with pytest.raises(_lib.TrunetHipError):
        evaluate(x, x)                                      # CPU tensors
    with pytest.raises(_lib.TrunetHipError):
        evaluate(torch.zeros(2, 100), torch.zeros(2, 100), lengths=[100, 50], fs=48000)
    with pytest.raises(ValueError, match="utterance 0"):
        validate(None, [torch.zeros(1000)], [torch.zeros(999)])


def test_metric_entry_points_reject_null_and_inconsistent_totals():
    from tinyrecurrentunet_amd import _lib
    lib = _lib.lib()
    EINVAL = _lib.TRUNET_EINVAL
    a, b, io, oo, t = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    rs = lib.trunet_resample_ragged
    # one utterance of 16000 samples at 16 kHz -> 10000
    assert rs(None, b, io, oo, t, 290, 5, 8, 1, 16000, 10000, 2, None) == EINVAL
    assert rs(a, b, io, oo, None, 290, 5, 8, 1, 16000, 10000, 2, None) == EINVAL
    assert rs(a, b, io, oo, t, 290, 5, 65, 1, 16000, 10000, 2, None) == EINVAL        # q > 64
    assert rs(a, b, io, oo, t, 5000, 5, 8, 1, 16000, 10000, 2, None) == EINVAL        # too many taps
    assert rs(a, b, io, oo, t, 290, 5, 8, 0, 16000, 10000, 2, None) == EINVAL         # B = 0
    assert rs(a, b, io, oo, t, 290, 5, 8, 1, 16000, 10000, 3, None) == EINVAL         # three signals
    assert rs(a, b, io, oo, t, 290, 5, 8, 1, 16000, 10001, 2, None) == EINVAL         # not ceil(L p / q)
    assert rs(a, b, io, oo, t, 290, 5, 8, 1, 16000, 9999, 2, None) == EINVAL
    st = lib.trunet_stoi_ragged
    p = [0x1000 * (k + 1) for k in range(12)]
    # 10000 samples at 10 kHz: 77 frames, 47 segments, 1 workgroup
    good = (1, 10000, 77, 47, 1)
    for k in range(12):
        q = list(p)
        q[k] = None
        assert st(*q, *good, None) == EINVAL, k
    for bad in [(0, 10000, 77, 47, 1), (1, 10000, 79, 47, 1), (1, 10000, 77, 78, 2), (1, 10000, 77, 47, 0),
                (1, 10000, 77, 47, 2)]:
        assert st(*p, *bad, None) == EINVAL, bad
    sd = lib.trunet_si_sdr_ragged
    assert sd(None, b, io, oo, t, 0x6000, 1, 20000, 2, None) == EINVAL
    assert sd(a, b, io, oo, t, None, 1, 20000, 2, None) == EINVAL
    assert sd(a, b, io, oo, t, 0x6000, 1, 20000, 1, None) == EINVAL                   # chunks do not cover it
    assert sd(a, b, io, oo, t, 0x6000, 1, 20000, 3, None) == EINVAL
    assert sd(a, b, io, oo, t, 0x6000, 0, 20000, 2, None) == EINVAL
    assert lib.trunet_stoi_workspace_bytes(0, 10, 1) == 0
    assert lib.trunet_stoi_workspace_bytes(3, 77, 47) >= 77 * (8 + 4 + 2 * 15 * 4) + 3 * 4 + 2 * 47 * 8


def test_evaluate_command_line_help_and_errors(tmp_path):
    r = subprocess.run([sys.executable, "-m", "tinyrecurrentunet_amd.evaluate", "--help"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for opt in ("--clean", "--enhanced", "--noisy", "--json", "--max-seconds", "PESQ is not computed"):
        assert opt in " ".join(r.stdout.split()), opt
    r = subprocess.run([sys.executable, "-m", "tinyrecurrentunet_amd.evaluate", "--clean", str(tmp_path / "nope"),
                        "--enhanced", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "not a folder" in r.stderr
    r = subprocess.run([sys.executable, "-m", "tinyrecurrentunet_amd.evaluate", "--clean", str(tmp_path),
                        "--enhanced", str(tmp_path), "--max-seconds", "0"], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "max-seconds" in r.stderr
