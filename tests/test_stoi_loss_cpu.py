"""The intelligibility loss without a GPU: the torch restatement (tests/stoi_loss_ref.py) against the numpy definition
(tests/metrics_ref.py) and against finite differences, the conditions the GPU tests' fixtures must meet, and the host-side
argument checks of stoi_loss.py and of the new entry points."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import metrics_ref as M
import stoi_loss_cases as SC
import stoi_loss_ref as R


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_restatement_forward_equals_the_numpy_definition(name):
    fs, _, _, _, _, K, segs = SC.CASES[name]
    y, x = SC.pair(name)
    m = M.stoi_ref(x.double().numpy(), y.double().numpy(), fs)
    assert (m["kept"], m["segments"]) == (K, segs)
    assert m["margin_db"] >= SC.MARGIN_DB
    for ext, key in ((False, "stoi"), (True, "estoi")):
        r = R.score(y.double(), x.double(), fs, ext)
        assert (r["kept"], r["segments"]) == (K, segs)
        assert abs(float(r["score"]) - m[key]) <= 1e-12, (name, key, float(r["score"]), m[key])


@pytest.mark.parametrize("extended", [False, True])
def test_gradcheck_of_the_float64_restatement(extended):
    y, x = SC.pair("k31_16k")
    y64 = y.double().requires_grad_(True)
    # 64 of the 6758 samples carry the perturbation, spread over the utterance: the full Jacobian costs minutes
    idx = torch.arange(50, y.shape[0], y.shape[0] // 64)[:64]

    def f(d):
        return R.score(y64.detach().index_add(0, idx, d), x.double(), 16000, extended)["score"]
    d0 = torch.zeros(idx.shape[0], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(f, (d0,), eps=1e-6, atol=1e-9, rtol=1e-5)


def test_stoi_fixtures_keep_their_clip_decisions_in_fp32_and_one_of_them_clips():
    shares = {}
    for name in SC.GRAD_CASES:
        r = SC.ref(name, False)
        if r["r64"]["first"] is None:
            continue
        f64, f32 = r["r64"]["first"], r["r32"]["first"]
        differ = float((f64 != f32).double().mean())
        shares[name] = float((~f64).double().mean())
        print("%s: clip active on %.2f %% of the cells, fp32 / fp64 decisions differ on %.3f %%"
              % (name, 100 * shares[name], 100 * differ))
        assert differ <= 1e-3, (name, differ)
    assert max(shares.values()) >= 0.01, shares


@pytest.mark.parametrize("extended", [False, True])
def test_tail_fixture_keeps_the_sign_of_the_l1_term(extended):
    """the L1 gradient is sign(audio - clean): no sample of the tail fixture may sit so close to its clean value that fp32
    rounding decides the sign (16 times the fp32 restatement's own error is the margin asked for)"""
    r64, r32 = SC.tail_ref(extended, torch.float64), SC.tail_ref(extended, torch.float32)
    clean = SC.tail_inputs()[1].double()
    e32 = float((r32["audio"].double() - r64["audio"]).abs().max())
    assert float((r64["audio"] - clean).abs().min()) > 16 * e32
    assert torch.equal(torch.sign(r64["audio"] - clean), torch.sign(r32["audio"].double() - clean))


def test_argument_errors_without_a_device():
    from tinyrecurrentunet_amd import _lib
    from tinyrecurrentunet_amd.stoi_loss import STOILoss
    x = [torch.zeros(1000), torch.zeros(500)]
    f = STOILoss()
    with pytest.raises(ValueError, match="utterance 1"):
        f([torch.zeros(1000), torch.zeros(499)], x)
    with pytest.raises(ValueError, match="2 clean and 1"):
        f(x[:1], x)
    with pytest.raises(ValueError, match="44.1 kHz"):
        STOILoss(fs=44100)
    with pytest.raises(ValueError):
        STOILoss(fs=0)
    with pytest.raises(ValueError, match="lengths"):
        f(torch.zeros(2, 100), torch.zeros(2, 100), lengths=[100, 101])
    with pytest.raises(ValueError, match="no utterance"):
        f([], [])
    with pytest.raises(_lib.TrunetHipError):
        f(x, x)                                             # CPU tensors
    with pytest.raises(_lib.TrunetHipError):
        STOILoss(extended=True, fs=48000)(torch.zeros(2, 100), torch.zeros(2, 100), lengths=[100, 50])


def test_loss_fn_refuses_unknown_stoi_settings_before_the_network_runs():
    from tinyrecurrentunet_amd import util

    class Net(torch.nn.Module):
        def forward(self, feats):
            raise AssertionError("the network ran")
    X = (torch.zeros(1, 1, 1024), torch.zeros(1, 1, 1024))
    with pytest.raises(ValueError, match="stoi_config"):
        util.loss_fn(Net(), X, 1, 1, 0, None, pcen=False, stoi_lambda=1.0, stoi_config={"fs": 8000})


def test_entry_points_reject_null_and_inconsistent_totals():
    from tinyrecurrentunet_amd import _lib
    lib = _lib.lib()
    EINVAL = _lib.TRUNET_EINVAL
    bw = lib.trunet_stoi_loss_bwd
    p = [0x1000 * (k + 1) for k in range(11)]
    # 10000 samples at 10 kHz: 77 frames, 47 segments, 1 workgroup
    good = (1, 10000, 77, 47, 1)
    for k in range(11):
        q = list(p)
        q[k] = None
        assert bw(*q, -1.0, 0, 0x9000, *good, None) == EINVAL, k
    assert bw(*p, -1.0, 0, None, *good, None) == EINVAL                                 # no gradient buffer
    assert bw(*p, -1.0, 2, 0x9000, *good, None) == EINVAL                               # extended is 0 or 1
    assert bw(*p, float("nan"), 0, 0x9000, *good, None) == EINVAL
    for bad in [(0, 10000, 77, 47, 1), (1, 10000, 79, 47, 1), (1, 10000, 77, 78, 2), (1, 10000, 77, 47, 0),
                (1, 10000, 77, 47, 2), (1, -1, 0, 0, 0)]:
        assert bw(*p, -1.0, 0, 0x9000, *bad, None) == EINVAL, bad
    rb = lib.trunet_resample_ragged_bwd
    a, b, io, oo, t = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    assert rb(None, b, io, oo, t, 290, 5, 8, 1, 16000, 10000, None) == EINVAL
    assert rb(a, None, io, oo, t, 290, 5, 8, 1, 16000, 10000, None) == EINVAL
    assert rb(a, b, io, oo, None, 290, 5, 8, 1, 16000, 10000, None) == EINVAL
    assert rb(a, b, io, oo, t, 290, 5, 65, 1, 16000, 10000, None) == EINVAL           # q > 64
    assert rb(a, b, io, oo, t, 5000, 5, 8, 1, 16000, 10000, None) == EINVAL           # too many taps
    assert rb(a, b, io, oo, t, 290, 5, 8, 0, 16000, 10000, None) == EINVAL            # B = 0
    assert rb(a, b, io, oo, t, 290, 5, 8, 1, 16000, 10001, None) == EINVAL            # not ceil(L p / q)
    lv = lib.trunet_stoi_loss_value
    assert lv(None, 2, 1.0, 0x2000, None, None) == EINVAL
    assert lv(0x1000, 2, 1.0, None, None, None) == EINVAL
    assert lv(0x1000, 0, 1.0, 0x2000, None, None) == EINVAL
    assert lv(0x1000, 2, float("nan"), 0x2000, None, None) == EINVAL
    assert lib.trunet_stoi_loss_workspace_bytes(0, 10, 1) == 0
    assert lib.trunet_stoi_loss_workspace_bytes(3, 77, 47) >= 47 * 450 * 8 + 77 * (15 * 8 + 4 + 256 * 4)
