"""Offline enhancement (tinyrecurrentunet_amd/enhance.py) without a GPU: argument validation raises before any launch, the
ragged entry points refuse what the host can see, and the command line parses."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(**kw):
    from tinyrecurrentunet_amd.network import TRUNet
    return TRUNet(input_size=4, **kw).eval()


def test_enhance_validation_errors_without_a_device():
    from tinyrecurrentunet_amd import _lib
    from tinyrecurrentunet_amd.enhance import enhance
    net = _net()
    ok = torch.zeros(1000)
    assert enhance(net, []) == []
    assert net.enhance([]) == []
    with pytest.raises(ValueError, match="utterance 2 "):
        enhance(net, [ok, ok, torch.zeros(256), ok])
    with pytest.raises(_lib.TrunetHipError):
        enhance(net, [ok, torch.zeros(257)])                          # CPU tensors
    with pytest.raises(_lib.TrunetHipError):
        net.enhance(torch.zeros(2, 1000), lengths=[1000, 300])
    X = torch.zeros(3, 1000)
    with pytest.raises(ValueError, match="lengths"):
        enhance(net, X, lengths=[1000, 1001, 500])                   # longer than a row
    with pytest.raises(ValueError, match="lengths"):
        enhance(net, X, lengths=[1000, 500])                         # one length short
    with pytest.raises(ValueError, match="lengths"):
        enhance(net, [ok], lengths=[1000])                           # lengths belong to the padded form
    with pytest.raises(ValueError, match="utterance 1 "):
        enhance(net, X, lengths=[1000, 100, 500])
    with pytest.raises(ValueError):
        enhance(net, [ok], path="eager")
    with pytest.raises(ValueError):
        enhance(net, [ok], max_frames=0)
    with pytest.raises(ValueError):
        enhance(_net(use_tgru=True), [ok], path="folded")
    net.train()
    with pytest.raises(_lib.TrunetHipError, match="eval"):
        enhance(net, [ok])


def test_tgru_groups_bound_the_padding():
    from tinyrecurrentunet_amd.enhance import tgru_groups, TGRU_MIN_FILL
    frames = [126, 3, 501, 126, 250, 2000, 125, 126, 400]
    groups, pad = tgru_groups(frames, max_frames=600)
    assert sorted(i for g in groups for i in g) == list(range(len(frames)))
    for g in groups:
        tmax = frames[g[0]]
        assert all(frames[i] <= tmax and frames[i] >= TGRU_MIN_FILL * tmax for i in g)
        assert len(g) * tmax <= max(600, tmax)
    computed = sum(len(g) * frames[g[0]] for g in groups)
    assert abs(pad - (1 - sum(frames) / computed)) < 1e-12 and 0 <= pad < 1 - TGRU_MIN_FILL
    assert tgru_groups([1251] * 150, max_frames=8192) == ([list(range(i, min(i + 6, 150))) for i in range(0, 150, 6)], 0.0)


def test_ragged_entry_points_reject_null_and_inconsistent_totals():
    """The three ragged entry points validate what the host can see and return TRUNET_EINVAL before any launch."""
    from tinyrecurrentunet_amd import _lib
    lib = _lib.lib()
    EINVAL = _lib.TRUNET_EINVAL
    a, so, fo, po, f, m, tw = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
    # one utterance of 1000 samples: T = 8 frames, 4 pairs
    good = (1000, 8, 4)
    feat = lib.trunet_stft_features_ragged
    assert feat(None, so, fo, po, f, m, tw, 1, *good, 4, None) == EINVAL
    assert feat(a, None, fo, po, f, m, tw, 1, *good, 4, None) == EINVAL
    assert feat(a, so, None, po, f, m, tw, 1, *good, 4, None) == EINVAL
    assert feat(a, so, fo, None, f, m, tw, 1, *good, 4, None) == EINVAL
    assert feat(a, so, fo, po, None, m, tw, 1, *good, 4, None) == EINVAL
    assert feat(a, so, fo, po, f, m, None, 1, *good, 4, None) == EINVAL
    assert feat(a, so, fo, po, f, m, tw, 0, *good, 4, None) == EINVAL            # B <= 0
    assert feat(a, so, fo, po, f, m, tw, -3, *good, 4, None) == EINVAL
    assert feat(a, so, fo, po, f, m, tw, 1, *good, 5, None) == EINVAL            # C = 5
    assert feat(a, so, fo, po, f, m, tw, 1, *good, 2, None) == EINVAL
    for bad in [(256, 3, 2),            # fewer than 257 samples per utterance
                (1000, 2, 1),           # fewer than 3 frames per utterance
                (1000, 9, 5),           # more frames than 1 + L / 128
                (1000, 8, 3),           # fewer pairs than frames / 2
                (1000, 8, 5)]:          # more pairs than (frames + B) / 2
        assert feat(a, so, fo, po, f, m, tw, 1, *bad, 3, None) == EINVAL, bad
    assert feat(a, so, fo, po, f, m, tw, 4, 1000, 12, 6, 3, None) == EINVAL      # 1000 samples cannot hold 4 utterances
    ist = lib.trunet_mask_istft_ragged
    o, fr, au = 0x8000, 0x9000, 0xa000
    assert ist(None, fr, au, so, fo, po, tw, 1, *good, 0.5, None) == EINVAL
    assert ist(o, None, au, so, fo, po, tw, 1, *good, 0.5, None) == EINVAL
    assert ist(o, fr, None, so, fo, po, tw, 1, *good, 0.5, None) == EINVAL
    assert ist(o, fr, au, None, fo, po, tw, 1, *good, 0.5, None) == EINVAL
    assert ist(o, fr, au, so, None, po, tw, 1, *good, 0.5, None) == EINVAL
    assert ist(o, fr, au, so, fo, None, tw, 1, *good, 0.5, None) == EINVAL
    assert ist(o, fr, au, so, fo, po, None, 1, *good, 0.5, None) == EINVAL
    assert ist(o, fr, au, so, fo, po, tw, 0, *good, 0.5, None) == EINVAL
    assert ist(o, fr, au, so, fo, po, tw, 1, 1000, 9, 5, 0.5, None) == EINVAL
    assert ist(o, fr, au, so, fo, po, tw, 1, 1000, 8, 1, 0.5, None) == EINVAL
    pc = lib.trunet_pcen_ragged
    args = (1e-6, 0.025, 0.98, 2.0, 0.5, None)
    assert pc(None, f, fo, 1, 8, 4 * 257, *args) == EINVAL
    assert pc(m, None, fo, 1, 8, 4 * 257, *args) == EINVAL
    assert pc(m, f, None, 1, 8, 4 * 257, *args) == EINVAL
    assert pc(m, f, fo, 0, 8, 4 * 257, *args) == EINVAL
    assert pc(m, f, fo, 3, 2, 4 * 257, *args) == EINVAL                           # fewer frames than utterances
    assert pc(m, f, fo, 1, 8, 256, *args) == EINVAL                               # a row narrower than 257 bins


def test_enhance_command_line_help():
    r = subprocess.run([sys.executable, "-m", "tinyrecurrentunet_amd.enhance", "--help"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for opt in ("--checkpoint", "--input-size", "--use-tgru", "--in", "--out", "--max-seconds"):
        assert opt in r.stdout
