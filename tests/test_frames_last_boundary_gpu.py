"""The frames-last boundary of the train step (fft.hip: trunet_stft_features_fl, trunet_pcen_fl, trunet_mask_istft_fwd_fl,
trunet_mask_istft_bwd_fl; util.loss_fn -> TRUNet -> the fused loss node through ``_lib.FramesLast``) is a pure layout change:
everything here is compared with torch.equal against the (N, C, 257) entry points and trunet_to_frames_last.

Shapes: (B 3, L 512): T = 5 (odd: every utterance ends in a half pair, pairs straddle the 32-frame groups at odd offsets),
N = 15 in NP = 256 (one group is half padding, seven are all padding); (B 2, L 16640): T = 131, N = 262 in NP = 512 (the group
128..159 holds the end of utterance 0 and the start of utterance 1, N crosses a 256-frame tile)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
SHAPES = [(3, 512), (2, 16640)]
BINS = 257
# two small resolutions: the reflect padding of the STFT loss needs L > n / 2 at L = 512
CFG = dict(fft_sizes=[512, 256], hop_sizes=[128, 64], win_lengths=[480, 240], sc_lambda=0.5, mag_lambda=0.5, band="full")


def _dims(B, L):
    T = 1 + L // 128
    N = B * T
    return T, N, (N + 255) // 256 * 256


def _to_fl(x, NP):
    """trunet_to_frames_last: (N, C, 257) -> [C][257][NP]"""
    from tinyrecurrentunet_amd import _lib as Lb
    N, C, Ln = x.shape
    y = torch.full((C, Ln, NP), float("nan"), device="cuda")
    Lb.check(Lb.lib().trunet_to_frames_last(Lb.ptr(x), Lb.ptr(y), N, C, Ln, NP, Lb.stream()), "to_frames_last")
    return y


def _net_out(B, L, seed):
    """a random network output in both layouts: [8][257][NP] with NaN padding columns (nobody may read them), (N, 8, 257).
    Scale 1.5: channel 0 leaves the clamp's [-1, 1] on both sides; a few phase pairs are exactly (0, 0)."""
    T, N, NP = _dims(B, L)
    g = torch.Generator().manual_seed(seed)
    o = 1.5 * torch.randn(N, 8, BINS, generator=g)
    o[::3, 2:4, ::5] = 0.0
    o[1::4, 6:8, 1::7] = 0.0
    o = o.cuda()
    fl = torch.full((8, BINS, NP), float("nan"), device="cuda")
    fl[:, :, :N] = o.permute(1, 2, 0)
    return o.contiguous(), fl.contiguous()


@pytest.mark.parametrize("pcen", [False, True])
@pytest.mark.parametrize("B,L", SHAPES)
def test_features_frames_last(B, L, pcen):
    from tinyrecurrentunet_amd import _lib as Lb, dataset as ds
    T, N, NP = _dims(B, L)
    C = 4 if pcen else 3
    audio = torch.randn(B, L, generator=torch.Generator().manual_seed(L + C)).cuda()
    ref = _to_fl(ds.stft_features(audio, pcen=pcen), NP)
    lib, st = Lb.lib(), Lb.stream()
    x = torch.full((C, BINS, NP), float("nan"), device="cuda")
    mag = torch.full((BINS, NP), float("nan"), device="cuda") if pcen else None
    tw = Lb.twiddles(512, audio.device)
    Lb.check(lib.trunet_stft_features_fl(Lb.ptr(audio), Lb.ptr(x), Lb.ptr(mag), Lb.ptr(tw), B, L, T, C, NP, st), "features_fl")
    if pcen:
        Lb.check(lib.trunet_pcen_fl(Lb.ptr(mag), Lb.ptr(x[1]), B, T, NP, 1e-6, 0.025, 0.98, 2.0, 0.5, st), "pcen_fl")
    assert not torch.isnan(x).any()
    assert torch.equal(x[:, :, N:], torch.zeros_like(x[:, :, N:]))
    for c in range(C):
        assert torch.equal(x[c], ref[c]), c
    h = ds.stft_features(audio, pcen=pcen, _frames_last=True)
    assert h.N == N and torch.equal(h.t, ref)


@pytest.mark.parametrize("B,L", SHAPES)
def test_mask_istft_forward_frames_last(B, L):
    from tinyrecurrentunet_amd import _lib as Lb
    T, N, NP = _dims(B, L)
    o, o_fl = _net_out(B, L, seed=L)
    clean = torch.randn(B, L, generator=torch.Generator().manual_seed(1)).cuda()
    lib, st = Lb.lib(), Lb.stream()
    tw = Lb.twiddles(512, clean.device)
    npart = lib.trunet_mask_istft_l1_nparts(B, L)
    res = []
    for fl in (False, True):
        frames = torch.full((B, T, 512), float("nan"), device="cuda")
        audio = torch.full((B, L), float("nan"), device="cuda")
        part = torch.full((npart,), float("nan"), device="cuda")
        tail = (Lb.ptr(frames), Lb.ptr(audio), Lb.ptr(clean), Lb.ptr(part), Lb.ptr(tw), B, T, L)
        if fl:
            Lb.check(lib.trunet_mask_istft_fwd_fl(Lb.ptr(o_fl), *tail, NP, 0.5, st), "mask_istft_fwd_fl")
        else:
            Lb.check(lib.trunet_mask_istft_fwd(Lb.ptr(o), *tail, 0.5, st), "mask_istft_fwd")
        res.append((frames, audio, part))
    for name, a, b in zip(("frames", "audio", "l1 partials"), *res):
        assert not torch.isnan(a).any(), name
        assert torch.equal(a, b), name


@pytest.mark.parametrize("B,L", SHAPES)
def test_mask_istft_backward_frames_last(B, L):
    from tinyrecurrentunet_amd import _lib as Lb
    T, N, NP = _dims(B, L)
    o, o_fl = _net_out(B, L, seed=L + 1)
    g_audio = torch.randn(B, L, generator=torch.Generator().manual_seed(2)).cuda()
    lib, st = Lb.lib(), Lb.stream()
    tw = Lb.twiddles(512, g_audio.device)
    g = torch.full((N, 8, BINS), float("nan"), device="cuda")
    Lb.check(lib.trunet_mask_istft_bwd(Lb.ptr(g_audio), Lb.ptr(o), Lb.ptr(g), Lb.ptr(tw), B, T, L, 0.5, st), "mask_istft_bwd")
    g_fl = torch.full((8, BINS, NP), float("nan"), device="cuda")
    Lb.check(lib.trunet_mask_istft_bwd_fl(Lb.ptr(g_audio), Lb.ptr(o_fl), Lb.ptr(g_fl), Lb.ptr(tw), B, T, L, NP, 0.5, st),
             "mask_istft_bwd_fl")
    assert not torch.isnan(g).any() and float(g.abs().max()) > 0
    assert torch.equal(g_fl[:, :, N:], torch.zeros_like(g_fl[:, :, N:]))
    assert torch.equal(g_fl[:, :, :N].permute(2, 0, 1), g)
    assert torch.equal(g_fl, _to_fl(g, NP))


def _step_setup(B, L, seed=3):
    from tinyrecurrentunet_amd import network as hn, stft_loss as sl
    torch.manual_seed(seed)
    net = hn.TRUNet(input_size=4)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    clean = 0.3 * torch.randn(B, 1, L, generator=g)
    noisy = clean + 0.1 * torch.randn(B, 1, L, generator=g)
    return state, (clean.cuda(), noisy.cuda()), sl.MultiResolutionSTFTLoss(**CFG).cuda()


def _spy_features(monkeypatch):
    """records whether util.loss_fn asked the front end for the frames-last hand-off"""
    from tinyrecurrentunet_amd import dataset as ds
    seen = []
    orig = ds.stft_features

    def spy(*a, **kw):
        seen.append(bool(kw.get("_frames_last", False)))
        return orig(*a, **kw)
    monkeypatch.setattr(ds, "stft_features", spy)
    return seen


@pytest.mark.parametrize("B,L", SHAPES)
def test_train_step_is_the_same_with_and_without_the_boundary(B, L, monkeypatch):
    from tinyrecurrentunet_amd import network as hn, util
    state, X, mr = _step_setup(B, L)
    seen = _spy_features(monkeypatch)
    res = []
    for env in (None, "0"):
        if env is None:
            monkeypatch.delenv("TRUNET_FL_BOUNDARY", raising=False)
        else:
            monkeypatch.setenv("TRUNET_FL_BOUNDARY", env)
        net = hn.TRUNet(input_size=4)
        net.load_state_dict(state)
        net.cuda().train()
        loss, info = util.loss_fn(net, X, ell_p=1, ell_p_lambda=1, stft_lambda=1, mrstftloss=mr)
        loss.backward()
        grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
        bufs = {n: b.clone() for n, b in net.named_buffers()}
        res.append((loss.detach().clone(), {k: v.clone() for k, v in info.items()}, grads, bufs))
    assert seen == [True, False]
    (l1, i1, g1, b1), (l0, i0, g0, b0) = res
    assert torch.isfinite(l1) and torch.equal(l1, l0)
    assert set(i1) == set(i0) == {"l1", "stft_sc", "stft_mag"}
    for k in i0:
        assert torch.equal(i1[k], i0[k]), k
    assert set(g1) == set(g0) and len(g0) > 90
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n
    assert float(max(g.abs().max() for g in g0.values())) > 0
    assert set(b1) == set(b0) and any("running_var" in n for n in b0)
    for n in b0:
        assert torch.equal(b1[n], b0[n]), n


def test_a_foreign_cotangent_gets_its_padding_zeroed():
    """Only the fused loss node's cotangent is known to have zero padding columns.  Any other gradient of the frames-last
    output -- here the all-ones of ``sum()``, padding included -- must give what the (N, 8, 257) path gives for it."""
    from tinyrecurrentunet_amd import dataset as ds, network as hn
    B, L = SHAPES[0]
    state, (_, noisy), _ = _step_setup(B, L)
    grads = []
    for fl in (True, False):
        net = hn.TRUNet(input_size=4)
        net.load_state_dict(state)
        net.cuda().train()
        out = net(ds.stft_features(noisy[:, 0].contiguous(), pcen=True, _frames_last=fl))
        if fl:
            assert out.N == _dims(B, L)[1] and out.t.shape == (8, BINS, _dims(B, L)[2])
            out = out.t
        out.sum().backward()
        grads.append({n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None})
    assert set(grads[0]) == set(grads[1]) and len(grads[0]) > 90
    for n in grads[0]:
        assert torch.isfinite(grads[0][n]).all() and torch.equal(grads[0][n], grads[1][n]), n


def test_second_forward_before_backward_is_refused(monkeypatch):
    """The hand-off's tensor is the recording workspace's output buffer: the loss node's backward reads it again, so it makes the
    workspace generation check first, and a training forward in between is refused like it is for the saved activations."""
    from tinyrecurrentunet_amd import _lib as Lb, network as hn, util
    monkeypatch.delenv("TRUNET_FL_BOUNDARY", raising=False)
    B, L = SHAPES[0]
    state, X, mr = _step_setup(B, L)
    seen = _spy_features(monkeypatch)
    net = hn.TRUNet(input_size=4)
    net.load_state_dict(state)
    net.cuda().train()
    first, _ = util.loss_fn(net, X, ell_p=1, ell_p_lambda=1, stft_lambda=1, mrstftloss=mr)
    with torch.no_grad():                                    # a forward that does not record leaves the buffer alone
        util.loss_fn(net, X, ell_p=1, ell_p_lambda=1, stft_lambda=1, mrstftloss=mr)
    second, _ = util.loss_fn(net, X, ell_p=1, ell_p_lambda=1, stft_lambda=1, mrstftloss=mr)
    assert seen == [True, False, True]
    with pytest.raises(Lb.TrunetHipError, match="overwritten"):
        first.backward()
    second.backward()
    assert all(torch.isfinite(p.grad).all() for p in net._active_params())
