"""CPU: the int8 artefact's exporter (tinyrecurrentunet_amd/quantize.py) -- the weight codes against fold()'s folded weights,
the fp32 sections bit for bit, the size against the paper's 362 KB, save / load and the refusals -- and the float64
restatement of its numerics (tests/quant_ref.py) against oracle/network_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quant_ref as qr  # noqa: E402

_NETS = {}


def _net(cin, seed=2, use_tgru=False):
    from oracle import network_ref as nr, weights as W
    from tinyrecurrentunet_amd import network as hn
    key = (cin, seed, use_tgru)
    if key not in _NETS:
        ref = W.fill_state_dict(nr.TRUNet(input_size=cin), seed=seed)
        net = hn.TRUNet(input_size=cin, use_tgru=use_tgru)
        net.load_state_dict(ref.state_dict())
        _NETS[key] = net.eval()
    return _NETS[key]


def _artefact(cin):
    from tinyrecurrentunet_amd.quantize import QuantizedTRUNet
    return QuantizedTRUNet.from_module(_net(cin), device="cpu")


@pytest.mark.parametrize("cin", [3, 4])
def test_codes_and_scales_against_the_folded_weights(cin):
    from tinyrecurrentunet_amd import export as E, quantize as Q
    blob, offs, _ = E.fold(_net(cin))
    secs = Q._folded_sections(blob, offs)
    sec = _artefact(cin).dequantized_sections()
    n_weights = 0
    for i, (M, K, t32) in Q._MATS.items():
        W, b = (E._unfrag_tiles if t32 else E._unfrag_tiles16)(secs[i], M, K)
        q, s, bq = sec[Q.SECTION_NAMES[i]]
        assert q.shape == (M, K) and q.dtype == np.int8 and s.dtype == np.float32
        deq = q.astype(np.float64) * s.astype(np.float64)[:, None]
        assert np.all(np.abs(deq - W) <= s.astype(np.float64)[:, None] / 2), Q.SECTION_NAMES[i]
        assert np.all(np.abs(q).max(1) == 127), Q.SECTION_NAMES[i]          # every row reaches its scale
        assert np.abs(q).max() <= 127
        assert np.array_equal(bq, b)                                         # folded biases stay fp32
        n_weights += M * K
    Ws, bhh = Q._whh_of_folded(secs[12])
    for (q, s), W in zip(sec["whh"], Ws):
        assert np.all(np.abs(q.astype(np.float64) * s.astype(np.float64)[:, None] - W) <= s.astype(np.float64)[:, None] / 2)
        assert np.all(np.abs(q).max(1) == 127)
        n_weights += q.size
    assert np.array_equal(sec["bhh"], bhh)
    assert n_weights == 287_744
    # fp32 sections: fold()'s values bit for bit
    for i, name in enumerate(Q.SECTION_NAMES):
        if i in Q._FP32:
            w, b = sec[name]
            n = Q._fp32_size(i, cin)
            assert np.array_equal(np.concatenate([w, b]).view(np.uint32), secs[i][:n].view(np.uint32)), name


def test_all_zero_rows():
    from tinyrecurrentunet_amd.quantize import quantize_rows, _tiles_i8, _untiles_i8
    W = np.random.default_rng(0).standard_normal((20, 128))
    W[3] = 0.0
    W[17] = 0.0
    W[5] = 0.0
    W[5, 7] = -1e-30                                           # a tiny non-zero row still reaches +-127
    q, s = quantize_rows(W)
    assert s[3] == 0 and s[17] == 0 and not q[3].any() and not q[17].any()
    assert abs(int(q[5, 7])) == 127 and s[5] > 0
    b = np.arange(20, dtype=np.float32)
    q2, s2, b2 = _untiles_i8(_tiles_i8(q, s, b), 20, 128)      # 20 rows: a padded second tile
    assert np.array_equal(q2, q) and np.array_equal(s2, s) and np.array_equal(b2, b)


@pytest.mark.parametrize("cin", [3, 4])
def test_artefact_size_within_the_papers_362_kb(cin):
    from tinyrecurrentunet_amd.quantize import PAPER_BYTES
    a = _artefact(cin)
    assert a.nbytes <= PAPER_BYTES, a.nbytes
    assert a.nbytes < 0.32 * _folded_bytes(cin)


def _folded_bytes(cin):
    from tinyrecurrentunet_amd import export as E
    return 4 * len(E.fold(_net(cin))[0])


def test_save_load_round_trip_and_refusals(tmp_path):
    from tinyrecurrentunet_amd import _lib as L
    from tinyrecurrentunet_amd.export import FoldedTRUNet
    from tinyrecurrentunet_amd.quantize import QuantizedTRUNet, FORMAT
    a = _artefact(4)
    p = tmp_path / "q.pt"
    a.save(str(p))
    d = torch.load(str(p), weights_only=True)
    assert d["format"] == FORMAT == "trunet-int8-v1"
    b = QuantizedTRUNet.load(str(p), device="cpu")
    assert torch.equal(a.blob, b.blob) and np.array_equal(a.offsets, b.offsets) and b.cin == 4
    with pytest.raises(L.TrunetHipError):
        FoldedTRUNet.load(str(p))                             # the fp32 runner refuses the int8 format
    for fmt in ("trunet-folded-v3", "trunet-folded-v2"):
        torch.save(dict(d, format=fmt), str(tmp_path / "f.pt"))
        with pytest.raises(L.TrunetHipError):
            QuantizedTRUNet.load(str(tmp_path / "f.pt"))     # and this one the fp32 formats
    with pytest.raises(L.TrunetHipError, match="bounds"):
        QuantizedTRUNet(a.blob[:-4096], a.offsets, 4, device="cpu")     # truncated image: host check
    with pytest.raises(L.TrunetHipError):
        QuantizedTRUNet(a.blob, a.offsets[:25], 4, device="cpu")
    o = a.offsets.copy()
    o[3] += 2                                                 # misaligned section
    with pytest.raises(L.TrunetHipError, match="bounds"):
        QuantizedTRUNet(a.blob, o, 4, device="cpu")


def test_time_recurrent_block_is_refused():
    from tinyrecurrentunet_amd import _lib as L, export as E
    from tinyrecurrentunet_amd.quantize import QuantizedTRUNet, quantize, quantize_folded
    with pytest.raises(L.TrunetHipError):
        QuantizedTRUNet.from_module(_net(4), device="cpu", tgru=True)
    with pytest.raises(L.TrunetHipError):
        quantize(_net(4, use_tgru=True))
    with pytest.raises(L.TrunetHipError):
        quantize_folded(*E.fold(_net(4), tgru=True))


@pytest.mark.parametrize("cin", [3, 4])
def test_restatement_without_activation_quantization_is_the_oracle(cin):
    sec = _artefact(cin).dequantized_sections()
    x = torch.randn(5, cin, 257, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    with torch.no_grad():
        a = qr.forward(x, sec, act=False)
        b = qr.dequantized_net(sec, cin)(x)
        c = qr.forward(x, sec)
    assert float((a - b).abs().max()) <= 1e-12
    rel = float((c - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
    assert 1e-4 < rel < 5e-2, rel                            # activation quantization moves the output, but not far


def test_fake_quant_rule():
    x = torch.tensor([[[0.5, -1.0, 0.25]], [[0.0, 0.0, 0.0]], [[3.0, 1e-3, -2.0]]], dtype=torch.float64)
    y = qr.fake_quant(x)
    assert torch.equal(y[1], x[1])                            # amax = 0: all zeros
    assert float(y[0].abs().max()) == 1.0 and float(y[2].abs().max()) == 3.0
    assert float(y[2, 0, 1]) == 0.0                           # below half a code (3 / 254)
    assert float(y[0, 0, 2]) == pytest.approx(32 / 127)       # 0.25 * 127 = 31.75 -> 32
