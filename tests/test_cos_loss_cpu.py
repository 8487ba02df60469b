"""CPU: the host side of the time-domain loss terms: the repaired cosine loss R8 against the reference's
own value, what the reference cannot do (B > 1, a gradient), the segment helper, the validation of g, the drop-in import and
the entry points' argument checks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tinyrecurrentunet_amd import _lib
from tinyrecurrentunet_amd import cos_loss as cl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("length", [4224, 2944])
def test_cos_sim_loss_reproduces_the_reference_value_for_one_row(golden, length):
    """tests/golden/cos_loss.npz: the unmodified reference CosSimLoss() on B = 1; L = 2944 clips the last segment"""
    g = golden("cos_loss")
    x, y = torch.from_numpy(g["x_%d" % length]), torch.from_numpy(g["y_%d" % length])
    want = float(g["loss_%d" % length])
    got = float(cl.CosSimLoss()(x, y))
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)


def test_cos_sim_loss_takes_a_batch_and_has_a_gradient():
    rng = np.random.default_rng(3)
    y = torch.tensor(0.1 * rng.standard_normal((3, 4224)) + 0.01, dtype=torch.float32)
    x = (y + torch.tensor(0.05 * rng.standard_normal((3, 4224)), dtype=torch.float32)).requires_grad_(True)
    loss = cl.CosSimLoss()(x, y)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    assert torch.isfinite(x.grad).all() and float(x.grad[:, :4062].abs().max()) > 0
    assert float(x.grad[:, 4062:].abs().max()) == 0          # the default g covers the first 4062 samples only
    # float64 autograd of the definition, segment by segment
    x64 = x.detach().double().requires_grad_(True)
    b = [0, 508, 1016, 2032, 4062]
    ref = sum((1 - torch.nn.functional.cosine_similarity(x64[:, s:e], y.double()[:, s:e], dim=1, eps=1e-5)).mean()
              for s, e in zip(b, b[1:])) / 4
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) < 1e-6 * float(ref.detach())
    assert float((x.grad.double() - x64.grad).abs().max()) < 1e-5 * float(x64.grad.abs().max())


def test_si_sdr_loss_on_the_cpu_matches_the_metric_definition():
    rng = np.random.default_rng(4)
    y = torch.tensor(0.1 * rng.standard_normal((2, 3000)) + 0.01, dtype=torch.float64)
    x = (y + 0.03 * torch.tensor(rng.standard_normal((2, 3000)))).requires_grad_(True)
    loss = cl.SISDRLoss(eps=0.0)(x, y)
    xm, ym = (x - x.mean(1, keepdim=True)).detach(), y - y.mean(1, keepdim=True)
    s = (xm * ym).sum(1, keepdim=True) / (ym * ym).sum(1, keepdim=True) * ym
    want = (10 * torch.log10((s * s).sum(1) / ((xm - s) ** 2).sum(1))).mean()
    assert abs(float(loss) + float(want)) < 1e-9 * abs(float(want))
    loss.backward()
    assert torch.isfinite(x.grad).all()
    # a constant target row contributes nothing and stays finite
    y0 = y.clone()
    y0[1] = 0.25
    x0 = x.detach().clone().requires_grad_(True)
    l0 = cl.SISDRLoss()(x0, y0)
    l0.backward()
    assert torch.isfinite(l0) and torch.isfinite(x0.grad).all() and float(x0.grad[1].abs().max()) == 0


def test_uniform_tiles_the_requested_length():
    m = cl.CosSimLoss.uniform(504, 8064)
    assert m.g[0] == 504 and m.g[-1] == 8064 and m.m == 16 and all(b - a == 504 for a, b in zip(m.g, m.g[1:]))
    m = cl.CosSimLoss.uniform(500, 1234)
    assert m.g == [500, 1000, 1234]
    assert cl.CosSimLoss.uniform(5000, 1234).g == [1234]
    assert cl.CosSimLoss().g == [508, 1016, 2032, 4062] and cl.CosSimLoss().eps == 1e-5


@pytest.mark.parametrize("g", [[], None, [0, 5], [-3, 5], [5, 5], [8, 4], list(range(1, 1027)), ["a"]])
def test_g_is_validated_on_the_host(g):
    with pytest.raises(ValueError):
        cl.CosSimLoss(g=g)


def test_g_accepts_the_largest_table():
    assert cl.CosSimLoss(g=list(range(1, 1025))).m == 1024
    with pytest.raises(ValueError):
        cl.CosSimLoss.uniform(0, 100)
    with pytest.raises(ValueError):
        cl.SISDRLoss(eps=-1.0)


def test_dropin_cos_loss_resolves_in_a_fresh_interpreter():
    lines = ["from cos_loss import CosSimLoss",                                                       # the reference's name
             "from cos_loss import SISDRLoss",
             "import cos_loss, tinyrecurrentunet_amd.cos_loss as impl; assert cos_loss.CosSimLoss is impl.CosSimLoss",
             "import torch; x = torch.randn(2, 600); v = CosSimLoss(eps=1e-5, g=[100, 300, 600])(x, x + 0.1)",
             "assert v.dim() == 0",
             # a reference-style loss_config carrying the new keys binds to loss_fn
             "from util import loss_fn; import inspect",
             "inspect.signature(loss_fn).bind(None, (None, None), ell_p=1, ell_p_lambda=1, stft_lambda=1, mrstftloss=None, "
             "cos_lambda=0.5, cos_config={'eps': 1e-5, 'g': [508, 1016]}, si_sdr_lambda=0.01, si_sdr_eps=1e-8)",
             "print('imports ok')"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dropin"), ROOT]))
    out = subprocess.run([sys.executable, "-c", "\n".join(lines)], env=env, capture_output=True, text=True, timeout=300,
                         cwd=str(ROOT))
    assert out.returncode == 0 and "imports ok" in out.stdout, out.stderr[-3000:]


def _call_fwd(lib, **kw):
    B, Ln, nseg = kw.pop("B", 2), kw.pop("Ln", 4224), kw.pop("nseg", 4)
    need = lib.trunet_wave_loss_workspace_bytes(2, 4224, 4)
    p = dict(audio=0x10000000, clean=0x20000000, bounds=0x30000000, seg_first=0x30001000, items=0x30002000, ws=0x40000000,
             vals=0x50000000, terms=0x50001000, coef=0x50002000, loss=None, ws_bytes=need, n_items=7)
    p.update(kw)
    a = _lib.WaveLossArgs()
    a.audio, a.clean, a.bounds, a.seg_first, a.items = p["audio"], p["clean"], p["bounds"], p["seg_first"], p["items"]
    a.B, a.L, a.nseg, a.n_items = B, Ln, nseg, p["n_items"]
    a.cos_lambda, a.si_sdr_lambda, a.cos_eps, a.si_sdr_eps = 1.0, 1.0, p.get("cos_eps", 1e-5), 1e-8
    return lib.trunet_wave_loss_fwd(a, p["ws"], p["ws_bytes"], p["vals"], p["terms"], p["coef"], p["loss"], None), a


def test_wave_loss_entry_points_validate_before_any_launch():
    lib = _lib.lib()
    EINVAL = _lib.TRUNET_EINVAL
    need = lib.trunet_wave_loss_workspace_bytes(2, 4224, 4)
    assert need > 0 and need % 8 == 0
    for name in ("audio", "clean", "bounds", "seg_first", "items", "ws", "vals", "terms", "coef"):
        assert _call_fwd(lib, **{name: None})[0] == EINVAL, name
    assert _call_fwd(lib, nseg=1025)[0] == EINVAL and _call_fwd(lib, nseg=-1)[0] == EINVAL
    assert _call_fwd(lib, B=0)[0] == EINVAL and _call_fwd(lib, B=-2)[0] == EINVAL and _call_fwd(lib, B=65536)[0] == EINVAL
    assert _call_fwd(lib, Ln=0)[0] == EINVAL and _call_fwd(lib, Ln=-7)[0] == EINVAL
    assert _call_fwd(lib, ws_bytes=need - 1)[0] == EINVAL and _call_fwd(lib, ws_bytes=0)[0] == EINVAL
    assert _call_fwd(lib, ws=0x40000004)[0] == EINVAL                                 # misaligned workspace
    assert _call_fwd(lib, n_items=0)[0] == EINVAL and _call_fwd(lib, n_items=2 * 3 + 4 + 1)[0] == EINVAL
    assert _call_fwd(lib, cos_eps=-1.0)[0] == EINVAL
    # written buffers may not overlap anything else
    assert _call_fwd(lib, ws=0x10000000)[0] == EINVAL and _call_fwd(lib, terms=0x20000000 + 4 * 4224)[0] == EINVAL
    assert _call_fwd(lib, coef=0x50001000)[0] == EINVAL and _call_fwd(lib, vals=0x30000000)[0] == EINVAL
    assert _call_fwd(lib, loss=0x50000010)[0] == EINVAL
    # the gradient entry point
    a = _call_fwd(lib, B=0)[1]
    a.B = 2

    def grad(a, coef=0x50002000, g_loss=0x60000000, g=0x70000000):
        return lib.trunet_wave_loss_grad(a, coef, g_loss, g, None)
    assert grad(None) == EINVAL and grad(a, coef=None) == EINVAL and grad(a, g_loss=None) == EINVAL and grad(a, g=None) == EINVAL
    assert grad(a, g=0x10000000) == EINVAL and grad(a, g=0x20000000 + 8) == EINVAL and grad(a, g=0x50002000) == EINVAL
    for field, bad in (("B", 0), ("L", 0), ("nseg", 1025), ("n_items", 0), ("audio", None), ("bounds", None)):
        keep = getattr(a, field)
        setattr(a, field, bad)
        assert grad(a) == EINVAL, field
        setattr(a, field, keep)


def test_wave_loss_workspace_bytes():
    f = _lib.lib().trunet_wave_loss_workspace_bytes
    assert f(0, 4224, 4) == 0 and f(-1, 4224, 4) == 0 and f(65536, 4224, 4) == 0
    assert f(2, 0, 4) == 0 and f(2, -5, 4) == 0 and f(2, (1 << 30) + 1, 4) == 0
    assert f(2, 4224, -1) == 0 and f(2, 4224, 1025) == 0
    assert f(2, 4224, 0) > 0 and f(2, 4224, 1024) > f(2, 4224, 4) > f(1, 4224, 4)
    assert f(2, 4224, 4) == 2 * (2 * 3 + 4) * 5 * 8                                   # rows x items x 5 fp64 sums
    assert f(64, 64000, 127) < 1 << 20
