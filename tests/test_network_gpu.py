"""GPU parity of the HIP TRU-Net body vs the oracle and the golden vectors (through the C ABI)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _errs(g, ref):
    g, ref = g.detach().double().cpu(), ref.detach().double().cpu()
    d = g - ref
    return float(d.abs().max()), float(d.norm()), float(ref.abs().max()), float(ref.norm())


def _grad_close(g, ref, name, errs=None):
    """Gradient parity metric.  A weight-gradient element is a sum of ~N*L products gated by ReLU
    masks, and BatchNorm makes several of these sums strongly cancelling, so fp32 rounding is
    amplified in EVERY fp32 implementation.  Measured vs the fp64 oracle (N=300,
    scripts/dbg/grad_precision.py, relative L2 per tensor, median / max over the 100 tensors):
    HIP 2.9e-3 / 1.2e-2, torch CPU fp32 4.7e-3 / 6.4e-3, torch GPU fp32 1.2e-2 / 2.5e-2; over seeds 3,4,5 the
    medians are HIP 1.0e-2, 6.8e-3, 4.3e-3 vs torch GPU fp32 1.2e-2, 6.4e-3, 4.0e-3 (a single flip near the
    output perturbs every tensor below it, so the whole vector of errors moves together from run to run).
    Bounds: 6e-2 relative L2 for every tensor (the bound that pins the arithmetic) and 8e-2 of max|g| per
    element (single elements of the cancelling BatchNorm-gamma sums move by a few % between ANY two
    summation orders, e.g. 256 vs 512 partial rows); callers also bound the median.  Conv biases in front of a BatchNorm have an analytically zero gradient (rounding
    noise in the reference), hence the absolute floors."""
    emax, el2, rmax, rl2 = _errs(g, ref)
    assert emax < 8e-2 * rmax + 2e-3, (name, emax, rmax)
    assert el2 < 6e-2 * rl2 + 2e-3, (name, el2, rl2)
    if errs is not None and rmax > 1e-3:
        errs.append(el2 / rl2)


def _nets(cin, seed=0):
    from oracle import network_ref as nr, weights as W
    from tinyrecurrentunet_amd import network as hn
    ref = W.fill_state_dict(nr.TRUNet(input_size=cin), seed=seed)
    net = hn.TRUNet(input_size=cin)
    net.load_state_dict(ref.state_dict())
    return ref, net.cuda()


@pytest.mark.parametrize("cin", [3, 4])
def test_forward_matches_golden(golden, cin):
    """north_star bar: forward within 1e-4 relative fp32 of the reference composition."""
    g = golden("trunet_cin%d" % cin)
    _, net = _nets(cin)
    x = torch.tensor(g["x"]).cuda()
    net.eval()
    with torch.no_grad():
        y = net(x)
    assert _rel(y, torch.tensor(g["y_eval"])) < 1e-4
    net.train()
    y = net(x)
    assert _rel(y, torch.tensor(g["y_train"])) < 1e-4
    mse = float(((y.cpu() - torch.tensor(g["y_train"])) ** 2).mean())
    assert mse < 1e-4


@pytest.mark.parametrize("cin", [3, 4])
def test_backward_matches_golden(golden, cin):
    g = golden("trunet_cin%d" % cin)
    _, net = _nets(cin)
    net.train()
    y = net(torch.tensor(g["x"]).cuda())
    (y * torch.tensor(g["cot"]).cuda()).sum().backward()
    n = 0
    for pn, p in net.named_parameters():
        if pn.startswith("TGRU"):
            assert p.grad is None
            continue
        ref = torch.tensor(g["g:" + pn])
        n += p.numel()
        _grad_close(p.grad, ref, pn)
    assert n == int(g["n_grad_params"])
    for bn_, b in net.named_buffers():
        if b.is_floating_point() and not bn_.startswith("TGRU"):
            assert _rel(b, torch.tensor(g["buf:" + bn_])) < 1e-4, bn_


@pytest.mark.parametrize("N", [1, 126, 300])
def test_forward_backward_vs_oracle_f64(N):
    """Ragged frame counts (not multiples of the 128-frame tile), vs the fp64 oracle."""
    from oracle import network_ref as nr, weights as W
    ref, net = _nets(4, seed=3)
    refd = W.fill_state_dict(nr.TRUNet(input_size=4), seed=3).double()
    x = torch.tensor(np.random.default_rng(N).standard_normal((N, 4, 257)) * 0.5, dtype=torch.float32)
    cot = torch.tensor(np.random.default_rng(N + 1).standard_normal((N, 8, 257)), dtype=torch.float32)
    refd.eval(); net.eval()
    with torch.no_grad():
        assert _rel(net(x.cuda()), refd(x.double())) < 1e-4
    if N == 1:
        return    # BatchNorm training statistics need more than one value per channel
    refd.train(); net.train()
    yd = refd(x.double()); (yd * cot.double()).sum().backward()
    errs = []
    y = net(x.cuda()); (y * cot.cuda()).sum().backward()
    assert _rel(y, yd) < 1e-4
    pd = dict(refd.named_parameters())
    for pn, p in net.named_parameters():
        if pn.startswith("TGRU"):
            continue
        ref_g = pd[pn].grad
        _grad_close(p.grad, ref_g, pn, errs)
    assert float(np.median(errs)) < 2.5e-2, float(np.median(errs))

@pytest.mark.parametrize("switch", ["FUSED_PWBWD", "FUSED_CONVT", "FUSED_THIN", "FUSED_GRU_PROJ"])
def test_unfused_fallback_schedules_through_trunet(switch, monkeypatch):
    """the separate-launch schedules the engine falls back to when a fused backward kernel answers
    TRUNET_ENOTSUP (engine._pw_bwd / _convt_bwd / the thin decoder.5 layer / the GRU input projection) driven once THROUGH
    TRUNet -- the same switches TRUNET_FUSED_PWBWD / _CONVT / _THIN / _GRU_PROJ = 0 set -- against the fused result on the
    same forward state: the backward is linear in the cotangent and both schedules multiply the same fp32 numbers, so they
    may differ by summation order only (conv biases in front of a BatchNorm: analytically zero, absolute floor)."""
    import tinyrecurrentunet_amd.engine as E
    ref, net = _nets(4, seed=5)
    N = 300
    x = torch.tensor(np.random.default_rng(N).standard_normal((N, 4, 257)) * 0.5, dtype=torch.float32).cuda()
    cot = torch.tensor(np.random.default_rng(N + 1).standard_normal((N, 8, 257)), dtype=torch.float32).cuda()

    def grads():
        net.zero_grad(set_to_none=True)
        net.load_state_dict(ref.state_dict())
        net.train()
        y = net(x)
        (y * cot).sum().backward()
        return y.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}

    y1, fused = grads()
    assert getattr(E, switch) is True
    monkeypatch.setattr(E, switch, False)
    y0, sep = grads()
    monkeypatch.undo()
    assert torch.equal(y0, y1)
    assert set(sep) == set(fused) and sum(t.numel() for t in sep.values()) == 298592
    worst, differs = 0.0, False
    for n, a in fused.items():
        b = sep[n]
        differs |= not torch.equal(a, b)
        sib = n[:-6] + "bias" if n.endswith(".1.weight") else (n[:-4] + "weight" if n.endswith("bias") else n)
        scale = max(b.norm().item(), sep[sib].norm().item() if sib in sep else 0.0)
        e = (a - b).norm().item() / (scale + 1e-30)
        worst = max(worst, e)
        assert e < 2e-3, (switch, n, e)
    assert differs, "%s = False took the same launches as the fused schedule" % switch
    print("%s: unfused vs fused schedule, worst relative L2 over the gradient tensors %.2e" % (switch, worst))


def test_zero_batchnorm_weights_vs_oracle_f64():
    """pw_bwd_kernel takes the ReLU mask and the z of the source's BatchNorm-backward sums from the ACTIVATION it has
    staged in LDS (a = c0 z + c1 where a > 0, z = (a - c1) / c0) instead of reading the source a second time.  A
    BatchNorm weight of exactly zero (c0 = 0) leaves no z in a: those channels take the kernel's slow path (z from
    global memory).  Zeroed here: single channels and a whole 32-channel row tile of BatchNorms that feed the
    128 -> 128 encoder layers and the 64 + 128 -> 64 decoder layers; every gradient (the zeroed weights' own first)
    against the fp64 oracle."""
    from oracle import network_ref as nr, weights as W
    N = 126
    ref, net = _nets(4, seed=5)
    refd = W.fill_state_dict(nr.TRUNet(input_size=4), seed=5).double()
    zeroed = {"encoder.1.DepthwiseSeparableConv1d.4.weight": list(range(32, 64)),
              "encoder.2.DepthwiseSeparableConv1d.4.weight": [5, 77],
              "encoder.4.DepthwiseSeparableConv1d.4.weight": [127],
              "decoder.1.TrCNN.4.weight": [3, 40],
              "decoder.3.TrCNN.4.weight": [63]}
    with torch.no_grad():
        for m in (refd, net):
            pd = dict(m.named_parameters())
            for pn, idx in zeroed.items():
                pd[pn][idx] = 0.0
    x = torch.tensor(np.random.default_rng(N).standard_normal((N, 4, 257)) * 0.5, dtype=torch.float32)
    cot = torch.tensor(np.random.default_rng(N + 1).standard_normal((N, 8, 257)), dtype=torch.float32)
    refd.train(); net.train()
    yd = refd(x.double()); (yd * cot.double()).sum().backward()
    y = net(x.cuda()); (y * cot.cuda()).sum().backward()
    assert _rel(y, yd) < 1e-4
    pd = dict(refd.named_parameters())
    errs = []
    for pn, p in net.named_parameters():
        if pn.startswith("TGRU"):
            continue
        _grad_close(p.grad, pd[pn].grad, pn, errs)
        if pn in zeroed:
            g, r = p.grad.detach().double().cpu(), pd[pn].grad
            idx = zeroed[pn]
            if len(idx) > 8:      # (a single channel with beta <= 0 is masked out altogether: gradient exactly zero)
                assert float(r[idx].abs().max()) > 1e-2 * float(r.abs().max()), pn      # zeroed channels do have a gradient
            assert float((g[idx] - r[idx]).abs().max()) < 5e-2 * float(r.abs().max()), (pn, g[idx], r[idx])
    assert float(np.median(errs)) < 2.5e-2, float(np.median(errs))


@pytest.mark.parametrize("N,C,Ln", [(300, 4, 257), (1, 8, 257), (130, 3, 257), (77, 5, 13), (64, 8, 16)])
def test_layout_changes_between_the_module_boundary_and_frames_last(N, C, Ln):
    """trunet_to_frames_last / trunet_from_frames_last: (N, C, L) of the module API <-> [C][L][NP] with zero padding frames.
    Ragged N, tiles past the end of both axes, C * L with and without a factor of 4.  (A 64 x 64-tile variant with 16-byte
    accesses on both sides passed this test and measured no different in the step -- these three launches are 0.35 ms of 48 --
    so the 32 x 32 kernels stayed.)"""
    from tinyrecurrentunet_amd import _lib as L
    from tinyrecurrentunet_amd._lib import check, ptr
    lib, st = L.lib(), L.stream()
    NP = (N + 127) // 128 * 128
    x = torch.randn(N, C, Ln, device="cuda")
    y = torch.full((C, Ln, NP), float("nan"), device="cuda")
    check(lib.trunet_to_frames_last(ptr(x), ptr(y), N, C, Ln, NP, st), "to_frames_last")
    ref = torch.zeros(C, Ln, NP, device="cuda")
    ref[:, :, :N] = x.permute(1, 2, 0)
    assert torch.equal(y, ref)
    back = torch.full((N, C, Ln), float("nan"), device="cuda")
    check(lib.trunet_from_frames_last(ptr(y), ptr(back), N, C, Ln, NP, st), "from_frames_last")
    assert torch.equal(back, x)


def test_state_dict_keys_match_reference_layout():
    from oracle import network_ref as nr
    from tinyrecurrentunet_amd import network as hn
    a, b = nr.TRUNet(3).state_dict(), hn.TRUNet(3).state_dict()
    assert list(a) == list(b) and len(b) == 177
    assert all(a[k].shape == b[k].shape for k in a)


def test_cpu_tensor_fails_loudly():
    from tinyrecurrentunet_amd import network as hn, _lib
    with pytest.raises(_lib.TrunetHipError):
        hn.TRUNet(3)(torch.zeros(2, 3, 257))


BLOCKS = {
    "std": ("StandardConv1d", (4, 64, 5, 2)),
    "dsc_k3s1": ("DepthwiseSeparableConv1d", (64, 128, 3, 1)),
    "dsc_k5s2": ("DepthwiseSeparableConv1d", (128, 128, 5, 2)),
    "dsc_k3s2": ("DepthwiseSeparableConv1d", (128, 128, 3, 2)),
    "gru_bi": ("GRUBlock", (128, 64, 64, True)),
    "gru_uni": ("GRUBlock", (64, 128, 64, False)),
    "first_tr": ("FirstTrCNN", (64, 64, 3, 2)),
    "tr_k5s2": ("TrCNN", (192, 64, 5, 2)),
    "tr_k3s1": ("TrCNN", (192, 64, 3, 1)),
    "last_tr": ("LastTrCNN", (128, 8, 5, 2)),
}


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_block_forward_matches_reference_golden(golden, name):
    """Stand-alone block classes (network.py:9-120) vs outputs of the reference's own classes."""
    from oracle import weights as W
    from tinyrecurrentunet_amd import network as hn
    g = golden("block_" + name)
    cls, args = BLOCKS[name]
    mod = getattr(hn, cls)(*args)
    W.fill_state_dict(mod, seed=11)
    assert abs(W.checksum(mod) - float(g["wsum"])) < 1e-6 * float(g["wsum"])
    mod.cuda()
    ins = [torch.tensor(g["x%d" % i]).cuda() for i in range(2) if "x%d" % i in g]
    mod.eval()
    assert _rel(mod(*ins), torch.tensor(g["y_eval"])) < 1e-4
    mod.train()
    assert _rel(mod(*ins), torch.tensor(g["y_train"])) < 1e-4
    for bn_, b in mod.named_buffers():
        if b.is_floating_point():
            assert _rel(b, torch.tensor(g["buf:" + bn_])) < 1e-4, bn_


def _zero_grad_biases(mod):
    """names of conv biases that sit directly in front of a BatchNorm: their gradient is analytically zero (the
    BatchNorm subtracts the mean), so the reference holds rounding noise there and there is nothing to compare"""
    out = set()
    for mn, m in mod.named_modules():
        if isinstance(m, torch.nn.Sequential):
            for i in range(len(m) - 1):
                if isinstance(m[i + 1], torch.nn.BatchNorm1d) and getattr(m[i], "bias", None) is not None:
                    out.add((mn + "." if mn else "") + "%d.bias" % i)
    return out


def _tight(g, ref, name, tol, zero=(), outliers=0.0, maxf=3.0, zero_floor=2e-2):
    """Relative L2 AND max-abs error, both relative to the tensor's own scale (no absolute floor).
    ``outliers``: fraction of elements left out of both bounds (largest errors first).  An fp32 and an fp64 run of a
    ReLU network disagree on the mask of the few pre-activations that lie within rounding error of zero (about one in
    1e6-1e7); each such flip changes an O(1) gradient contribution and spreads over the ~100 data-gradient elements
    that share the position.  Only data gradients of the large-N tests use it; a dropped tap, a wrong offset or a
    missing share of a sum moves (nearly) every element and is not masked by it."""
    g, ref = g.detach().double().cpu(), torch.as_tensor(ref).double()
    scale = float(ref.abs().max())
    if name in zero:
        # rounding noise of a sum of ~N*L O(1) terms that cancels exactly (fp32 partial sums of magnitude ~N*L)
        assert float(g.abs().max()) < zero_floor and scale < zero_floor, (name, float(g.abs().max()), scale)
        return
    d = (g - ref).abs().reshape(-1)
    if outliers > 0:
        k = d.numel() - int(outliers * d.numel())
        d = torch.topk(d, k, largest=False).values
    assert float(d.norm() / ref.norm()) < tol, (name, "L2", float(d.norm() / ref.norm()))
    assert float(d.max()) < maxf * tol * scale, (name, "max", float(d.max()), scale)


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_block_backward_matches_reference_golden(golden, name):
    """Backward of every stand-alone block class on the HIP path (the same launches the fused TRUNet schedule uses for
    that block: dwconv_bwd, gru_bwd / tgru_rec_bwd, transposed-conv dgrad + wgrad on tap segments with crop / pad,
    pw_bwd, bn_finalize_bwd, conv_first wgrad) against gradients produced by the REFERENCE's own classes
    (network.py:9-120 under torch autograd, tests/golden/make_golden.py): input gradients gx*, every parameter
    gradient g:*.  Two or three frames only, so the sums are short and well conditioned: bound 1e-3 relative."""
    from oracle import weights as W
    from tinyrecurrentunet_amd import network as hn
    g = golden("block_" + name)
    cls, args = BLOCKS[name]
    mod = getattr(hn, cls)(*args)
    W.fill_state_dict(mod, seed=11)
    mod.cuda().train()
    ins = [torch.tensor(g["x%d" % i]).cuda().requires_grad_(True) for i in range(2) if "x%d" % i in g]
    y = mod(*ins)
    assert _rel(y, torch.tensor(g["y_train"])) < 1e-4
    (y * torch.tensor(g["cot"]).cuda()).sum().backward()
    torch.cuda.synchronize()
    zero = _zero_grad_biases(mod)
    assert len(zero) == {"std": 0, "last_tr": 1, "gru_bi": 1, "gru_uni": 1}.get(name, 2)
    for i, x in enumerate(ins):
        assert x.grad is not None
        _tight(x.grad, g["gx%d" % i], "gx%d" % i, 1e-3)
    for pn, p in mod.named_parameters():
        assert p.grad is not None, pn
        _tight(p.grad, g["g:" + pn], pn, 1e-3, zero)


BLOCK_SHAPES = {   # input shapes per frame count N (the shapes these classes see inside TRUNet)
    "std": lambda N: [(N, 4, 257)],
    "dsc_k3s1": lambda N: [(N, 64, 32)],
    "dsc_k5s2": lambda N: [(N, 128, 31)],
    "dsc_k3s2": lambda N: [(N, 128, 32)],
    "gru_bi": lambda N: [(N, 16, 128)],
    "gru_uni": lambda N: [(N // 9, 9, 64)],
    "first_tr": lambda N: [(N, 64, 16)],
    "tr_k5s2": lambda N: [(N, 64, 31), (N, 128, 32)],      # F.pad by one on the left (decoder.1)
    "tr_k3s1": lambda N: [(N, 64, 66), (N, 128, 64)],      # crop one on each side (decoder.3's input, network.py:96-97)
    "last_tr": lambda N: [(N, 64, 130), (N, 64, 128)],
}


@pytest.mark.parametrize("N", [300, 777])
@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_block_backward_vs_oracle_f64(name, N):
    """Per-block backward at frame counts that span several tiles / partial rows and are not multiples of the tile
    width, against the fp64 oracle block (stock torch layers under autograd in double precision): every kernel of the
    backward schedule is pinned here on its own, with a short dependency chain: dwconv_bwd (k3s1, k5s2, k3s2), gru_bwd,
    tgru_rec_bwd, the transposed-conv data gradient / weight gradient launches on tap segments incl. F.pad and crop,
    pw_bwd, conv_first, relu_bwd_stats + bn_finalize_bwd.  Bounds, scaled to each tensor (no absolute floor): data
    gradients 2e-4 relative L2 outside the 1e-3 of elements hit by ReLU-mask flips (see _tight), parameter gradients
    1e-3 relative L2 and 1e-2 of max|g| per element (measured 2e-5 ... 8e-4; the whole-network bound was 6e-2)."""
    _block_vs_f64(name, N)


@pytest.mark.parametrize("name", ["dsc_k3s1", "dsc_k5s2", "dsc_k3s2", "tr_k3s1", "tr_k5s2", "first_tr", "gru_bi"])
def test_block_backward_vs_oracle_f64_at_8200_frames(name):
    """the same per-block comparison at a frame count beyond 8,192 (ragged: 8,200 = 64 tiles + 8 frames), where
    the persistent workgroups of pw_bwd_kernel (K = 64: dsc_k3s1; K = 128: dsc_k5s2 / dsc_k3s2; <32, true>: the decoder
    blocks), convt_bwd_kernel<3,1> / <5,2> / <3,2> and dw2_bwd_kernel<5,2> / <3,1> / <3,2> each walk many tiles, every
    partial weight-gradient image and statistics row is in use, and row offsets pass 2^20 floats."""
    # 10x the frames of the N = 777 case: the rounding noise of the analytically-zero bias sums grows with the square
    # root of the number of terms (floor 2e-2 -> 6.5e-2), and ~10x as many ReLU-mask flips between fp32 and fp64 land in
    # every parameter gradient (each moves it by ~3e-4 of its norm, in random directions: bound 1e-3 -> 2e-3; measured
    # worst case 1.1e-3, GRU.weight_ih_l0)
    _block_vs_f64(name, 8200, ptol=2e-3, zero_floor=2e-2 * (8200 / 777.0) ** 0.5)


@pytest.mark.parametrize("N", [1000, 8448])
def test_first_conv_backward_vs_oracle_f64_on_256_frame_chunks(N):
    """StandardConv1d (network.py:9-21) at frame counts whose padded size is a multiple of 256: the weight gradient runs on
    wgrad_first_kernel (round 3: one wave per SIMD, dz rows double-buffered in registers, x rows refilled per channel)
    instead of wgrad_small_kernel<4, 4, 5>; ragged N (frames >= N in the last chunk are zeroed), several items per block"""
    _block_vs_f64("std", N, ptol=1e-3 if N < 2000 else 2e-3)


@pytest.mark.parametrize("N", [1000, 8448])
def test_last_block_backward_vs_oracle_f64_on_256_frame_chunks(N):
    """LastTrCNN (network.py:102-120) at padded frame counts that are multiples of 256: the ConvTranspose1d(8 -> 8) weight
    gradient runs on wgrad_last_kernel and the data gradients of the 128 -> 8 pointwise layer on the 8-row-chunk
    conv_gemm instances (round 3)"""
    _block_vs_f64("last_tr", N, ptol=1e-3 if N < 2000 else 2e-3, zero_floor=2e-2 * max(1.0, N / 777.0) ** 0.5)


def _block_vs_f64(name, N, ptol=1e-3, zero_floor=2e-2):
    from oracle import network_ref as nr, weights as W
    from tinyrecurrentunet_amd import network as hn
    cls, args = BLOCKS[name]
    mod = W.fill_state_dict(getattr(hn, cls)(*args), seed=13).cuda().train()
    ref = W.fill_state_dict(getattr(nr, cls)(*args), seed=13).double().train()
    rng = np.random.default_rng(N + len(name))
    shapes = BLOCK_SHAPES[name](N)
    xs = [torch.tensor(rng.standard_normal(s) * 0.7, dtype=torch.float32) for s in shapes]
    xg = [x.cuda().requires_grad_(True) for x in xs]
    xd = [x.double().requires_grad_(True) for x in xs]
    y = mod(*xg)
    yd = ref(*xd)
    assert _rel(y, yd) < 1e-5
    cot = torch.tensor(rng.standard_normal(tuple(yd.shape)), dtype=torch.float32)
    (y * cot.cuda()).sum().backward()
    (yd * cot.double()).sum().backward()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(xg, xd)):
        _tight(a.grad, b.grad, "gx%d" % i, 2e-4, outliers=1e-3)
    pd = dict(ref.named_parameters())
    zero = _zero_grad_biases(mod)
    for pn, p in mod.named_parameters():
        # a single mask flip moves a weight gradient by ~3e-4 of its norm and one element by up to ~5e-3 of max|g|
        _tight(p.grad, pd[pn].grad, pn, ptol, zero, maxf=10.0 * 1e-3 / ptol, zero_floor=zero_floor)
    for bn_, b in mod.named_buffers():
        if b.is_floating_point():
            assert _rel(b, dict(ref.named_buffers())[bn_]) < 1e-5, bn_


def test_tgru_host_loop_schedule_vs_oracle_f64(monkeypatch):
    """TRUNET_TGRU_LOOP=1: the time loop as T (conv_gemm, tgru_cell_fwd_kernel) launch pairs forward and
    (tgru_cell_bwd_kernel, conv_gemm) pairs backward instead of the persistent tgru_rec_* kernels.  Same block, same
    inputs and the same bounds as test_block_backward_vs_oracle_f64[gru_uni-300]: the fallback schedule must be as right
    as the persistent one."""
    import tinyrecurrentunet_amd.engine as E
    assert E.TGRU_LOOP is False
    monkeypatch.setattr(E, "TGRU_LOOP", True)
    _block_vs_f64("gru_uni", 300)


def test_saved_activations_are_guarded():
    """activations saved for backward live in the engine's workspace.  A no_grad / eval forward between
    forward and backward must not disturb them (it runs in its own workspace); a second recording forward before the
    first backward must fail loudly instead of returning wrong gradients."""
    from tinyrecurrentunet_amd import _lib
    _, net = _nets(4, seed=5)
    net.train()
    x = torch.tensor(np.random.default_rng(0).standard_normal((40, 4, 257)) * 0.5, dtype=torch.float32).cuda()
    x2 = torch.tensor(np.random.default_rng(1).standard_normal((40, 4, 257)) * 0.5, dtype=torch.float32).cuda()
    cot = torch.tensor(np.random.default_rng(2).standard_normal((40, 8, 257)), dtype=torch.float32).cuda()
    y = net(x)
    (y * cot).sum().backward()
    ref = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    net.zero_grad()
    # BatchNorm running statistics moved in the first pass: reload so both passes see identical buffers
    _, net2 = _nets(4, seed=5)
    net2.train()
    y = net2(x)
    with torch.no_grad():
        net2(x2)                               # same padded frame count, would overwrite z:* in a shared workspace
        net2.eval(); net2(x2[:1]); net2.train()
    (y * cot).sum().backward()
    for n, p in net2.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, ref[n]), n
    y1 = net2(x)
    y2 = net2(x2)                              # second recording forward before the first backward
    with pytest.raises(_lib.TrunetHipError):
        (y1 * cot).sum().backward()
    (y2 * cot).sum().backward()                # the most recent forward is intact


@pytest.mark.parametrize("path", ["folded", "layers"])
@pytest.mark.parametrize("streams", [37, 300])
def test_tgru_streaming_matches_oracle(path, streams):
    """Stateful streaming with the TGRU block (network.py:150, rt.py:20-27): consecutive frames of
    `streams` streams, hidden state carried, vs the fp64 oracle's nn.GRU stepping (build-defined path: the reference never
    calls TGRU).  "folded": the whole step incl. the GRU time step in ONE launch (export.fold(tgru=True),
    stream_fwd_kernel<true>; 300 streams = more frames than workgroups, so a workgroup carries several streams);
    "layers": the layer-by-layer kernels (fold_eval = False)."""
    from oracle import network_ref as nr, weights as W
    ref, net = _nets(4, seed=7)
    refd = W.fill_state_dict(nr.TRUNet(input_size=4), seed=7).double().eval()
    net.eval()
    net.fold_eval = path == "folded"
    rng = np.random.default_rng(5)
    h, state = None, None
    for t in range(5):
        x = torch.tensor(rng.standard_normal((streams, 4, 257)) * 0.5, dtype=torch.float32)
        with torch.no_grad():
            yd, h = refd.stream_step(x.double(), h)
        y, state = net.stream_step(x.cuda(), state)
        assert _rel(y, yd) < 1e-4, (t, _rel(y, yd))
    assert state.steps == 5 and state.layout == ("folded" if path == "folded" else "frames_last")
    # hidden state parity: oracle h is (1, S*16, 128) with row s*16 + l
    hh = state.hidden().reshape(streams * 16, 128)
    assert _rel(hh, h[0]) < 1e-4
    with pytest.raises(Exception):
        net.stream_step(x.cuda()[:5], state)            # a state belongs to its number of streams
    with pytest.raises(Exception):
        net.train()
        net.stream_step(x.cuda(), state)


def test_folded_stream_step_replays_from_a_hip_graph():
    """the state keeps its address and is updated in place, so one captured step replays frame after frame
    (bench.py --streaming --tgru)"""
    from oracle import network_ref as nr, weights as W
    ref, net = _nets(4, seed=8)
    refd = W.fill_state_dict(nr.TRUNet(input_size=4), seed=8).double().eval()
    net.eval()
    rng = np.random.default_rng(6)
    xs = [torch.tensor(rng.standard_normal((64, 4, 257)) * 0.5, dtype=torch.float32) for _ in range(4)]
    xg = xs[0].cuda()
    y, state = net.stream_step(xg, None)                # frame 0 eagerly (builds the artefact and the state)
    with torch.no_grad():
        yd, h = refd.stream_step(xs[0].double(), None)
    assert _rel(y, yd) < 1e-4
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    keep = state.h.clone()
    with torch.cuda.graph(g):
        yg, _ = net.stream_step(xg, state)
    state.h.copy_(keep)                                  # capture does not execute; make sure of the starting state
    state.steps = 1
    for t in range(1, 4):
        xg.copy_(xs[t].cuda())
        g.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            yd, h = refd.stream_step(xs[t].double(), h)
        assert _rel(yg, yd) < 1e-4, t
    assert _rel(state.hidden().reshape(64 * 16, 128), h[0]) < 1e-4


@pytest.mark.parametrize("B,T", [(3, 7), (2, 40)])
def test_use_tgru_forward_backward_vs_oracle_f64(B, T):
    """TGRU as a trained layer (use_tgru=True): forward and every gradient (TGRU's included) vs the fp64 oracle."""
    from oracle import network_ref as nr, weights as W
    from tinyrecurrentunet_amd import network as hn
    refd = W.fill_state_dict(nr.TRUNet(input_size=4), seed=9).double()
    net = hn.TRUNet(input_size=4, use_tgru=True)
    net.load_state_dict(W.fill_state_dict(nr.TRUNet(input_size=4), seed=9).state_dict())
    net.cuda()
    N = B * T
    x = torch.tensor(np.random.default_rng(N).standard_normal((N, 4, 257)) * 0.5, dtype=torch.float32)
    cot = torch.tensor(np.random.default_rng(N + 1).standard_normal((N, 8, 257)), dtype=torch.float32)
    refd.eval(); net.eval()
    with torch.no_grad():
        assert _rel(net(x.cuda(), frames_per_seq=T), refd.forward_tgru(x.double(), T)) < 1e-4
    refd.train(); net.train()
    yd = refd.forward_tgru(x.double(), T)
    (yd * cot.double()).sum().backward()
    y = net(x.cuda(), frames_per_seq=T)
    assert _rel(y, yd) < 1e-4
    (y * cot.cuda()).sum().backward()
    pd = dict(refd.named_parameters())
    errs, n = [], 0
    for pn, p in net.named_parameters():
        assert p.grad is not None, pn
        n += p.numel()
        _grad_close(p.grad, pd[pn].grad, pn, errs)
    assert n == 381472                      # 381,472 parameters at C_in = 4 with TGRU
    assert float(np.median(errs)) < 2.5e-2, float(np.median(errs))
