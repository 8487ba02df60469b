"""GPU: offline enhancement of recordings of any lengths (tinyrecurrentunet_amd/enhance.py) -- the ragged front / back end
against the dense entry points on each utterance alone (bit for bit), the whole call against the float64 oracle
composition, against the stream and the util.denoise route, its invariance to batch-mates / order / chunking, the TGRU
padding, test-set scale and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [257, 258, 383, 384, 16000, 16001, 64127]


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _audio(lens, seed=0):
    g = np.random.default_rng(seed)
    return [torch.tensor(g.standard_normal(n) * 0.1, dtype=torch.float32).cuda() for n in lens]


_PAIRS = {}


def _pair(cin, seed=3, use_tgru=False, precision="fp32"):
    from oracle import network_ref as nr, weights as W
    from tinyrecurrentunet_amd import network as hn
    key = (cin, seed, use_tgru, precision)
    if key not in _PAIRS:
        ref = W.fill_state_dict(nr.TRUNet(input_size=cin), seed=seed).eval()
        net = hn.TRUNet(input_size=cin, use_tgru=use_tgru, precision=precision)
        net.load_state_dict(ref.state_dict())
        _PAIRS[key] = (ref, net.cuda().eval())
    return _PAIRS[key]


_ORACLE = {}


def _oracle(ref, cin, x, tgru=False):
    """features_ref -> oracle network (eval) -> denoise_from_output(length = L), all in float64 on the host"""
    from oracle import features_ref as fr
    key = (id(ref), cin, tgru, x.shape[0], float(x[:64].sum()))
    if key not in _ORACLE:
        xd = x.detach().double().cpu()
        T = 1 + xd.shape[0] // 128
        rd = ref.double()
        with torch.no_grad():
            feat = fr.features_batch(xd[None, None], pcen=(cin == 4))
            out = rd.forward_tgru(feat, T) if tgru else rd(feat)
            _ORACLE[key] = fr.denoise_from_output(out, T, beta=0.5, length=xd.shape[0])[0]
        ref.float()
    return _ORACLE[key]


@pytest.mark.parametrize("cin", [3, 4])
def test_ragged_features_and_pcen_bitwise_equal_the_dense_entry_points(cin):
    from tinyrecurrentunet_amd import dataset as ds, enhance as en
    xs = _audio(LENS, seed=cin)
    pk = en.Packed(xs, xs[0].device)
    feat = en.features(pk, cin)
    for b, x in enumerate(xs):
        f0, f1 = pk.offs[1, b], pk.offs[1, b + 1]
        ref = ds.stft_features(x[None], pcen=(cin == 4))
        assert torch.equal(feat[f0:f1], ref), (b, LENS[b], (feat[f0:f1] - ref).abs().max().item())
    # the equal-length batch: the dense entry point on all rows at once
    X = torch.stack(_audio([5000] * 5, seed=7))
    pk = en.Packed(list(X), X.device)
    assert torch.equal(en.features(pk, cin), ds.stft_features(X, pcen=(cin == 4)))


@pytest.mark.parametrize("cin", [3, 4])
def test_ragged_mask_istft_equals_the_dense_path_and_torch_istft(cin):
    from oracle import features_ref as fr
    from tinyrecurrentunet_amd import enhance as en, util
    _, net = _pair(cin)
    xs = _audio(LENS, seed=10 + cin)
    pk = en.Packed(xs, xs[0].device)
    with torch.no_grad():
        out = net.folded()(en.features(pk, cin))
        den = en.mask_istft(pk, out)
        for b, n in enumerate(LENS):
            f0, f1, s0 = pk.offs[1, b], pk.offs[1, b + 1], pk.offs[0, b]
            T = int(f1 - f0)
            got = den[s0:s0 + n]
            dense, _ = util.denoise(out[f0:f1], torch.zeros((1, (T - 1) * 128), device="cuda"), T)
            assert torch.equal(got[:(T - 1) * 128], dense[0]), (n, (got[:(T - 1) * 128] - dense[0]).abs().max().item())
            ref = fr.denoise_from_output(out[f0:f1].double().cpu(), T, beta=0.5, length=n)[0]
            assert _rel(got, ref) < 1e-5, (n, _rel(got, ref))


CASES = [(3, "fp32", "folded"), (4, "fp32", "folded"), (3, "fp32", "layers"), (4, "fp32", "layers"),
         (4, "bf16", "folded")]


@pytest.mark.parametrize("cin,precision,path", CASES)
def test_enhance_matches_the_float64_oracle(cin, precision, path):
    """every output has exactly its input's length and is within 1e-4 (max-abs / max-abs) of the float64 oracle
    composition; a bf16 net on path="folded" runs the same fp32 artefact as an fp32 net"""
    ref, net = _pair(cin, precision=precision)
    xs = _audio(LENS, seed=20 + cin)
    ys = net.enhance(xs, path=path)
    assert [y.shape[0] for y in ys] == LENS
    for x, y in zip(xs, ys):
        d = _rel(y, _oracle(ref, cin, x))
        assert d < 1e-4, (x.shape[0], d)
    if precision == "bf16":
        _, n32 = _pair(cin)
        for y, y32 in zip(ys, n32.enhance(xs, path="folded")):
            assert torch.equal(y, y32)


def test_bf16_net_on_the_layer_kernels_within_the_bf16_eval_gate():
    """path="layers" on a precision="bf16" net runs the bf16 eval schedule: gated like
    test_bf16_eval_forward_through_the_layer_kernels, 5e-2 relative L2 of the fp32 layer path (here on the audio)"""
    _, n16 = _pair(4, precision="bf16")
    _, n32 = _pair(4)
    xs = _audio(LENS, seed=31)
    y16 = torch.cat(n16.enhance(xs, path="layers"))
    y32 = torch.cat(n32.enhance(xs, path="layers"))
    assert torch.isfinite(y16).all()
    l2 = float((y16.double() - y32.double()).norm() / y32.double().norm())
    assert l2 < 5e-2, l2


@pytest.mark.parametrize("cin", [3, 4])
def test_enhance_equals_the_stream_and_the_util_denoise_route(cin):
    """L % 128 == 0: the existing streaming contract (1e-5) against AudioStream push + flush and against the offline
    route of the tests (stft_features -> net -> util.denoise with a dummy clean signal)"""
    from tinyrecurrentunet_amd import dataset as ds, util
    from tinyrecurrentunet_amd.streaming import AudioStream
    _, net = _pair(cin)
    S, hops = 3, 40
    X = torch.stack(_audio([128 * hops] * S, seed=40 + cin))
    Y = net.enhance(X)
    st = AudioStream(net, S)
    got = torch.cat([st.push(X[:, 128 * k:128 * (k + 1)].contiguous()) for k in range(hops)] + [st.flush()], 1)
    assert _rel(Y, got) < 1e-5, _rel(Y, got)
    with torch.no_grad():
        off, _ = util.denoise(net(ds.stft_features(X, pcen=(cin == 4))), torch.zeros_like(X), hops + 1)
    assert _rel(Y, off) < 1e-5, _rel(Y, off)


@pytest.mark.parametrize("path", ["folded", "layers"])
def test_enhance_is_invariant_to_batch_mates_order_and_chunking(path):
    """bit for bit for a fixed path: the folded kernel computes each frame in one workgroup, the eval-mode layer kernels
    have no cross-frame sums, and the ragged front / back end pair frames within an utterance only"""
    _, net = _pair(4)
    lens = LENS + [8000, 3001]
    xs = _audio(lens, seed=50)
    base = net.enhance(xs, path=path)
    perm = np.random.default_rng(1).permutation(len(xs)).tolist()
    shuf = net.enhance([xs[i] for i in perm], path=path)
    for k, i in enumerate(perm):
        assert torch.equal(shuf[k], base[i]), (path, lens[i], "order")
    mates = _audio([999, 20000, 4444], seed=51)
    other = net.enhance([mates[0], xs[4], mates[1], xs[6], mates[2], xs[0]], path=path)
    for k, i in ((1, 4), (3, 6), (5, 0)):
        assert torch.equal(other[k], base[i]), (path, lens[i], "mates")
    for mf in (1000, 8192, None):
        for y, yb in zip(net.enhance(xs, max_frames=mf, path=path), base):
            assert torch.equal(y, yb), (path, mf)


def test_tgru_net_on_ragged_lengths():
    """use_tgru: groups of B_g blocks of T_max frames with zero features after each end; every utterance within 1e-6 of
    the net on that utterance alone (frames_per_seq = T_b) and within 1e-4 of the oracle's forward_tgru composition"""
    from tinyrecurrentunet_amd import dataset as ds, enhance as en, util
    ref, net = _pair(4, seed=5, use_tgru=True)
    lens = LENS + [16100, 15000, 9000]
    xs = _audio(lens, seed=60)
    frames = [en.n_frames(n) for n in lens]
    groups, pad = en.tgru_groups(frames, max_frames=2048)
    assert len(groups) < len(lens) and any(len(g) > 1 for g in groups) and pad > 0
    ys = net.enhance(xs, max_frames=2048)
    assert [y.shape[0] for y in ys] == lens
    for x, y, T in zip(xs, ys, frames):
        with torch.no_grad():
            out = net(ds.stft_features(x[None], pcen=True), frames_per_seq=T)
        pk = en.Packed([x], x.device)
        alone = en.mask_istft(pk, out)
        assert _rel(y, alone) < 1e-6, (x.shape[0], _rel(y, alone))
        if x.shape[0] <= 16001:
            d = _rel(y, _oracle(ref, 4, x, tgru=True))
            assert d < 1e-4, (x.shape[0], d)


def test_list_form_equals_padded_form():
    _, net = _pair(3)
    xs = _audio(LENS, seed=70)
    ys = net.enhance(xs)
    Lmax = max(LENS)
    X = torch.zeros((len(xs), Lmax), device="cuda")
    for b, x in enumerate(xs):
        X[b, :x.shape[0]] = x
        X[b, x.shape[0]:] = 1.0                       # whatever lies past a length is not read
    Y = net.enhance(X, lengths=torch.tensor(LENS))
    assert Y.shape == (len(xs), Lmax)
    for b, y in enumerate(ys):
        assert torch.equal(Y[b, :LENS[b]], y)
        assert (Y[b, LENS[b]:] == 0).all()


@pytest.mark.parametrize("path", ["folded", "layers"])
def test_test_set_scale_equals_per_utterance_calls(path):
    """150 x 10 s (the DNS synthetic test-set shape) plus five odd lengths: ~190k frames in several network chunks, each
    utterance bit for bit its own enhance call"""
    _, net = _pair(4)
    lens = [160000] * 150 + [257, 12345, 64127, 33333, 99999]
    g = np.random.default_rng(80)
    xs = [torch.tensor(g.standard_normal(n) * 0.1, dtype=torch.float32).cuda() for n in lens]
    ys = net.enhance(xs, path=path)
    torch.cuda.synchronize()
    for b in list(range(0, 150, 7)) + list(range(150, 155)):
        assert torch.equal(ys[b], net.enhance([xs[b]], path=path)[0]), (path, b, lens[b])


def test_command_line_round_trip(tmp_path):
    from scipy.io.wavfile import read as wavread, write as wavwrite
    from tinyrecurrentunet_amd import dataset as ds
    _, net = _pair(4)
    ind, outd = tmp_path / "noisy", tmp_path / "clean"
    ind.mkdir()
    g = np.random.default_rng(90)
    names = {"a.wav": 16000, "b_odd.wav": 12345, "c.wav": 40000}
    for nm, n in names.items():
        wavwrite(str(ind / nm), 16000, (g.standard_normal(n) * 3000).astype(np.int16))
    ck = tmp_path / "ck.pkl"
    torch.save({"iter": 1, "model_state_dict": {k: v.cpu() for k, v in net.state_dict().items()}}, str(ck))
    r = subprocess.run([sys.executable, "-m", "tinyrecurrentunet_amd.enhance", "--checkpoint", str(ck), "--input-size", "4",
                        "--in", str(ind), "--out", str(outd), "--max-seconds", "3"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(outd)) == sorted(names)
    for nm, n in names.items():
        sr, q = wavread(str(outd / nm))
        assert sr == 16000 and q.dtype == np.int16 and q.shape == (n,)
        x, _ = ds._read_wav(str(ind / nm))
        y = net.enhance([x.cuda()])[0].cpu().numpy()
        ref = np.clip(np.round(y * 32768.0), -32768, 32767)
        assert np.abs(q.astype(np.int64) - ref).max() <= 1, nm
