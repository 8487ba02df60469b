"""The recurrence kernels of gru.hip (FGRU: trunet_gru_fwd / _bwd, both TRUNET_GRU_NE instances; TGRU: trunet_tgru_rec_fwd /
_bwd), the GRU cells and the sequence-major layout kernels of elementwise.hip, each on its own through the C ABI against
the fp64 restatement in tests/gru_ref.py -- at the kernels' own granularity (NP % 128, SP % 32), at L / T that end on either
LDS buffer, and at pre-activations where exp overflows and z (1 - z), 1 - n^2 vanish.  The tolerance of every comparison is
gru_ref.close: measured on the same inputs from the fp32 restatement's own error, never from the kernel's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gru_cases as G
import gru_ref as R

pytestmark = pytest.mark.gpu
ROOT = G.ROOT


def _id(case):
    return "-".join(str(v) for v in case)


# ---------------------------------------------------------------------------------------------- FGRU
@pytest.fixture(scope="module", params=G.FGRU_CASES, ids=_id)
def fgru(request):
    """inputs and the fp64 / fp32 references of one case, computed once and shared by the tests below (never modified)"""
    return G.fgru_refs(G.fgru_inputs(*request.param))


def test_fgru_forward(fgru):
    G.check_fgru_fwd(fgru)


def test_fgru_backward_on_the_reference_state(fgru):
    G.check_fgru_bwd(fgru, own=False)


def test_fgru_backward_on_the_forward_kernels_outputs(fgru):
    G.check_fgru_bwd(fgru, own=True)


@pytest.mark.parametrize("L,NP", [(16, 384), (17, 128)])
def test_fgru_backward_gradient_that_exists_only_through_the_carry(L, NP):
    """dhout is non-zero at a single position, the last one each direction visits: every dgi at the other positions is
    W_hh^T dgh and dh z carried back, nothing else"""
    c = G.fgru_refs(G.fgru_inputs("long", L, NP))
    dh = torch.zeros_like(c.dhout)
    dh[:G.FH, L - 1] = c.dhout[:G.FH, L - 1]
    dh[G.FH:, 0] = c.dhout[G.FH:, 0]
    r64 = R.fgru_bwd(dh, *c.state, c.whh, torch.float64)
    r32 = R.fgru_bwd(dh, *c.state, c.whh, torch.float32)
    dgi, dghn = G.gpu_fgru_bwd(dh, c.state[0], c.state[1], c.whh)
    G.compare(G.fgru_tag(c, "bwd(carry only)"), [("dgi", dgi, r64[0], r32[0]), ("dghn", dghn, r64[1], r32[1])])
    assert float(r64[0][:3 * G.FH, 0].abs().max()) > 0 and float(r64[0][3 * G.FH:, L - 1].abs().max()) > 0


def _fgru_all(gi, whh, bhh, dhout):
    hout, gates = G.gpu_fgru_fwd(gi, whh, bhh)
    dgi, dghn = G.gpu_fgru_bwd(dhout, hout, gates, whh)
    return {"hout": hout, "gates": gates, "dgi": dgi, "dghn": dghn}


def test_fgru_columns_are_independent():
    """Column n of every output is bit for bit the same whether the other columns hold zeros or the overflow regime, and
    whether the column sits in an NP = 128 or (at another lane and workgroup) an NP = 512 launch"""
    L = 16
    c = G.fgru_inputs("ordinary", L, 128)
    o = G.fgru_inputs("overflow", L, 512)
    base = _fgru_all(c.gi, c.whh, c.bhh, c.dhout)
    keep = torch.arange(128) % 3 == 0

    def embed(t, other, off, NP):
        out = other[..., :NP].clone()
        out[..., off:off + 128][..., keep] = t[..., keep]
        return out

    zero = lambda t: torch.zeros(t.shape[:-1] + (512,))
    over = lambda t: o.gi if t.shape[0] == 6 * G.FH else o.dhout * 200.0
    for name, (other, off, NP) in {"zeros": (zero, 0, 128), "overflow": (over, 0, 128), "NP512": (zero, 200, 512),
                                   "NP512+overflow": (over, 200, 512)}.items():
        got = _fgru_all(embed(c.gi, other(c.gi), off, NP), c.whh, c.bhh, embed(c.dhout, other(c.dhout), off, NP))
        for k, v in got.items():
            assert bool(torch.isfinite(v).all()), (name, k)
            assert torch.equal(v[..., off:off + 128][..., keep], base[k][..., keep]), (name, k)


def test_fgru_directions_are_independent():
    """zeroing one direction's W_hh and gi leaves the other direction's outputs bit-identical"""
    H = G.FH
    c = G.fgru_inputs("trained", 16, 128)
    base = _fgru_all(c.gi, c.whh, c.bhh, c.dhout)
    for d in range(2):
        gi, whh = c.gi.clone(), c.whh.clone()
        gi[d * 3 * H:(d + 1) * 3 * H] = 0
        whh[d] = 0
        got = _fgru_all(gi, whh, c.bhh, c.dhout)
        k = 1 - d
        assert torch.equal(got["hout"][k * H:(k + 1) * H], base["hout"][k * H:(k + 1) * H])
        assert torch.equal(got["gates"][k], base["gates"][k])
        assert torch.equal(got["dgi"][k * 3 * H:(k + 1) * 3 * H], base["dgi"][k * 3 * H:(k + 1) * 3 * H])
        assert torch.equal(got["dghn"][k * H:(k + 1) * H], base["dghn"][k * H:(k + 1) * H])
        assert not torch.equal(got["hout"][d * H:(d + 1) * H], base["hout"][d * H:(d + 1) * H])


_IN_PROCESS = {}


@pytest.mark.parametrize("ne", ["1", "2"])
def test_fgru_both_kernel_instances_in_a_fresh_interpreter(ne, tmp_path):
    """TRUNET_GRU_NE = 1 / 2 forces gru_fwd_kernel<NE> and gru_bwd_kernel<NE> (the default runs <2> forward and <1>
    backward, so <1> forward and <2> backward are launched by nothing else).  gru_ne() latches the environment at its
    first call: one child interpreter per value, one after the other, runs gru_cases.CHILD_CASES against the fp64 bounds
    and reports a checksum of every output tensor.  Both instances do the same operations per column in the same order,
    so the checksums must equal those of the in-process default."""
    out = str(tmp_path / "child.json")
    env = dict(os.environ, TRUNET_GRU_NE=ne)
    try:
        p = subprocess.run([sys.executable, "tests/gru_cases.py", out], cwd=ROOT, env=env, timeout=180,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    except subprocess.TimeoutExpired as e:
        pytest.fail("TRUNET_GRU_NE=%s child timed out:\n%s" % (ne, e.output))
    assert p.returncode == 0, "TRUNET_GRU_NE=%s child ended with %d:\n%s" % (ne, p.returncode, p.stdout[-4000:])
    child = json.load(open(out))
    assert child["TRUNET_GRU_NE"] == ne and len(child["sums"]) == len(G.CHILD_CASES)
    if not _IN_PROCESS:
        _IN_PROCESS.update(G.run_fgru_cases())
    diff = [(c, k) for c, s in _IN_PROCESS["sums"].items() for k in s if child["sums"][c][k] != s[k]]
    assert not diff, "TRUNET_GRU_NE=%s differs from the in-process default in %s" % (ne, diff)


# ---------------------------------------------------------------------------------------------- TGRU
@pytest.fixture(scope="module", params=G.TGRU_CASES, ids=_id)
def tgru(request):
    return G.tgru_refs(G.tgru_inputs(*request.param))


def test_tgru_forward(tgru):
    G.check_tgru_fwd(tgru)


def test_tgru_backward_on_the_reference_state(tgru):
    G.check_tgru_bwd(tgru, own=False)


def test_tgru_backward_on_the_forward_kernels_outputs(tgru):
    G.check_tgru_bwd(tgru, own=True)


def _tgru_all(gi, whh, bhn, dhs, S):
    hs, gates = G.gpu_tgru_fwd(gi, whh, bhn)
    dgi, dgh = G.gpu_tgru_bwd(dhs, hs, gates, whh, S)
    return {"hs": hs, "gates": gates, "dgi_all": dgi, "dgh_all": dgh}


def test_tgru_columns_are_independent():
    """as for FGRU: other columns zero or in the overflow regime, SP = 32 or (at another lane and workgroup) SP = 96"""
    T = 9
    c = G.tgru_inputs("ordinary", T, 32, 32)
    o = G.tgru_inputs("overflow", T, 96, 96)
    base = _tgru_all(c.gi, c.whh, c.bhn, c.dhs, 32)
    keep = torch.arange(32) % 3 == 0

    def embed(t, other, off, SP):
        out = other[..., :SP].clone()
        out[..., off:off + 32][..., keep] = t[..., keep]
        return out

    zero = lambda t: torch.zeros(t.shape[:-1] + (96,))
    over = lambda t: o.gi if t.shape[0] == 3 * G.TH else o.dhs * 200.0
    for name, (other, off, SP) in {"zeros": (zero, 0, 32), "overflow": (over, 0, 32), "SP96": (zero, 40, 96),
                                   "SP96+overflow": (over, 40, 96)}.items():
        got = _tgru_all(embed(c.gi, other(c.gi), off, SP), c.whh, c.bhn, embed(c.dhs, other(c.dhs), off, SP), SP)
        for k, v in got.items():
            assert bool(torch.isfinite(v).all()), (name, k)
            assert torch.equal(v[..., off:off + 32][..., keep], base[k][..., keep]), (name, k)


# ---------------------------------------------------------------------------------------------- cells
def _lib():
    from tinyrecurrentunet_amd import _lib as Lb
    return Lb


def test_tgru_cell_forward_one_step():
    """trunet_tgru_cell_fwd (the host-loop schedule's cell): step t = 2 of T = 4 writes hs[:, t + 1] and the gate planes of
    step t, nothing else"""
    Lb = _lib()
    H, T, t, SP = 128, 4, 2, 36
    g = G._gen("cellf")
    gi, gh = G._randn(g, 3 * H, T, SP) * 3, G._randn(g, 3 * H, SP) * 3
    hprev = torch.tanh(G._randn(g, H, SP))
    hs = G._nan(H, T + 1, SP)
    hs[:, t] = hprev.cuda()
    gates = G._nan(4, H, T, SP)
    gid, ghd = gi.cuda(), gh.cuda()
    Lb.check(Lb.lib().trunet_tgru_cell_fwd(Lb.ptr(gid), Lb.ptr(ghd), Lb.ptr(hs), Lb.ptr(gates), H, T, t, SP, Lb.stream()), "cell")
    torch.cuda.synchronize()
    hs, gates = hs.cpu(), gates.cpu()
    h64, g64 = R.gru_cell(gi[:, t], gh, hprev, torch.float64)
    h32, g32 = R.gru_cell(gi[:, t], gh, hprev, torch.float32)
    G.compare("TGRU cell fwd", [("h", hs[:, t + 1], h64, h32)] + [(n, gates[k, :, t], g64[k], g32[k])
                                                                 for k, n in enumerate(G.GATE_NAMES)])
    assert torch.equal(hs[:, t], hprev)
    rest = [i for i in range(T + 1) if i not in (t, t + 1)]
    assert bool(torch.isnan(hs[:, rest]).all()) and bool(torch.isnan(gates[:, :, [i for i in range(T) if i != t]]).all())


@pytest.mark.parametrize("with_carry", [False, True])
def test_tgru_cell_backward_one_step(with_carry):
    """trunet_tgru_cell_bwd with carry = NULL and a given carry, S < SP: the rows of step t of dgi_all / dgh_all, the direct
    path dhs[:, t] += dh z, exact zeros at the padded sequences although dhs holds NaN there"""
    Lb = _lib()
    H, T, t, SP, S = 128, 3, 1, 36, 30
    g = G._gen("cellb", with_carry)
    c = G.tgru_refs(G.tgru_inputs("trained", T, SP, S))
    hs, gates = c.state
    dhs = G._randn(g, H, T + 1, SP)
    dhs[:, t + 1, S:] = float("nan")
    carry = G._randn(g, H, SP) if with_carry else None
    dh = dhs[:, t + 1] + carry if with_carry else dhs[:, t + 1]          # fp32 sum, as the kernel forms it
    dh64 = dhs[:, t + 1].double() + carry.double() if with_carry else dhs[:, t + 1].double()
    zw = torch.zeros(3 * H, H)
    step = lambda d, dt: R.tgru_bwd(torch.stack((d, d), 1), hs[:, t:t + 2], gates[:, :, t:t + 1], zw, S, dt)
    r64, r32 = step(dh64, torch.float64), step(dh, torch.float32)
    live = (torch.arange(SP) < S)[None]
    z = gates[1, :, t]
    p64 = dhs[:, t].double() + torch.where(live, dh64, torch.zeros((), dtype=torch.float64)) * z.double()
    p32 = dhs[:, t] + torch.where(live, dh, torch.zeros(())) * z
    dhs_d, dgi, dgh = dhs.cuda(), G._nan(3 * H, T, SP), G._nan(3 * H, T, SP)
    carry_d = carry.cuda() if with_carry else None
    hs_d, gates_d = hs.cuda(), gates.cuda()          # named: a temporary's memory is reused by the next allocation
    Lb.check(Lb.lib().trunet_tgru_cell_bwd(Lb.ptr(dhs_d), Lb.ptr(carry_d), Lb.ptr(hs_d), Lb.ptr(gates_d), Lb.ptr(dgi),
                                           Lb.ptr(dgh), H, T, t, SP, S, Lb.stream()), "cell_bwd")
    torch.cuda.synchronize()
    dgi, dgh, dhs_o = dgi.cpu(), dgh.cpu(), dhs_d.cpu()
    G.compare("TGRU cell bwd carry=%s" % ("given" if with_carry else "NULL"),
              [("dgi", dgi[:, t], r64[0][:, 0], r32[0][:, 0]), ("dgh", dgh[:, t], r64[1][:, 0], r32[1][:, 0]),
               ("dhs[t]", dhs_o[:, t], p64, p32)])
    assert bool((dgi[:, t, S:] == 0).all()) and bool((dgh[:, t, S:] == 0).all())
    assert torch.equal(dhs_o[:, t, S:], dhs[:, t, S:]) and torch.equal(dhs_o[:, t + 1, :S], dhs[:, t + 1, :S])
    assert bool(torch.isnan(dgi[:, [0, 2]]).all()) and bool(torch.isnan(dgh[:, [0, 2]]).all())


def test_streaming_gru_cell_in_place():
    """trunet_gru_cell with h aliasing h_new, as the streaming TGRU step calls it"""
    Lb = _lib()
    H, Lg, NP = 128, 3, 36
    g = G._gen("cell")
    gi, gh = G._randn(g, 3 * H, Lg, NP) * 3, G._randn(g, 3 * H, Lg, NP) * 3
    h = torch.tanh(G._randn(g, H, Lg, NP))
    hd, gid, ghd = h.cuda(), gi.cuda(), gh.cuda()
    Lb.check(Lb.lib().trunet_gru_cell(Lb.ptr(gid), Lb.ptr(ghd), Lb.ptr(hd), Lb.ptr(hd), H, Lg, NP, Lb.stream()), "gru_cell")
    torch.cuda.synchronize()
    G.compare("streaming GRU cell", [("h", hd.cpu(), R.gru_cell(gi, gh, h, torch.float64)[0],
                                      R.gru_cell(gi, gh, h, torch.float32)[0])])


# ---------------------------------------------------------------------------------------------- layout kernels
@pytest.mark.parametrize("B,T", [(1, 1), (33, 33), (3, 70), (40, 2)])
def test_sequence_major_layout_kernels(B, T):
    """frames-last x[c][l][b T + t] <-> sequence-major y[c][t][b Lf + l].  Raw: a pure permutation, bit for bit both ways.
    `to` with BatchNorm+ReLU: the fp64 formula rounded to fp32 within 1 ulp.  `from` with the ReLU mask: elementwise against
    the fp64 mask, its partial sums against fp64 sums.  What `to` leaves at the padded sequences s >= S: zeros, and what
    `from` leaves at the padded frames: untouched memory."""
    Lb = _lib()
    lib, st = Lb.lib(), Lb.stream()
    C, Lf = 3, 16
    N, S = B * T, B * Lf
    NP, SP = N + 3, (S + 32) // 32 * 32              # ragged frame padding; at least one padded sequence
    g = G._gen("layout", B, T)
    x = G._randn(g, C, Lf, NP)
    to_seq = lambda v: v[:, :, :N].reshape(C, Lf, B, T).permute(0, 3, 2, 1).reshape(C, T, S)
    # to, raw
    xd, y = x.cuda(), G._nan(C, T, SP)
    Lb.check(lib.trunet_to_seq_major(Lb.ptr(xd), Lb.ptr(y), None, None, 0, C, Lf, T, B, NP, SP, st), "to")
    y = y.cpu()
    assert torch.equal(y[:, :, :S], to_seq(x))
    assert bool((y[:, :, S:] == 0).all()), "sequences >= S are not zero after trunet_to_seq_major"
    # to, BatchNorm + ReLU of the source
    sc, sh, mean = G._randn(g, C), G._randn(g, C) * 0.5, G._randn(g, C) * 0.3
    scd, shd, meand = sc.cuda(), sh.cuda(), mean.cuda()
    y2 = G._nan(C, T, SP)
    Lb.check(lib.trunet_to_seq_major(Lb.ptr(xd), Lb.ptr(y2), Lb.ptr(scd), Lb.ptr(shd), 1, C, Lf, T, B, NP, SP, st), "to")
    y2 = y2.cpu()
    pre = sc.double()[:, None, None] * x.double() + sh.double()[:, None, None]
    ref = to_seq(pre.clamp_min(0).float())
    ulps = (y2[:, :, :S].contiguous().view(torch.int32) - ref.contiguous().view(torch.int32)).abs()
    assert int(ulps.max()) <= 1, int(ulps.max())
    assert bool((y2[:, :, S:] == 0).all())
    # from, raw: the inverse permutation; frames >= N are not written
    ys = G._randn(g, C, T, SP)
    ysd = ys.cuda()
    back = G._nan(C, Lf, NP)
    Lb.check(lib.trunet_from_seq_major(Lb.ptr(ysd), Lb.ptr(back), None, None, None, None, None, C, Lf, T, B, NP, SP, st), "from")
    back = back.cpu()
    assert torch.equal(to_seq(back), ys[:, :, :S]) and bool(torch.isnan(back[:, :, N:]).all())
    # from, masked by the source's BatchNorm + ReLU, with the BatchNorm-backward partial sums
    nparts = lib.trunet_from_seq_major_nparts(Lf, T, B)
    part = G._nan(nparts, C, 2)
    xm = G._nan(C, Lf, NP)
    Lb.check(lib.trunet_from_seq_major(Lb.ptr(ysd), Lb.ptr(xm), Lb.ptr(xd), Lb.ptr(scd), Lb.ptr(shd), Lb.ptr(meand), Lb.ptr(part), C, Lf, T, B, NP, SP, st), "from")
    torch.cuda.synchronize()
    xm, part = xm.cpu(), part.cpu()
    yf = torch.zeros(C, Lf, N)
    yf.copy_(ys[:, :, :S].reshape(C, T, B, Lf).permute(0, 3, 2, 1).reshape(C, Lf, N))
    want = torch.where(pre[:, :, :N] > 0, yf, torch.zeros(()))
    sure = pre[:, :, :N].abs() >= 1e-6
    assert float((~sure).double().mean()) <= 1e-3
    assert torch.equal(xm[:, :, :N][sure], want[sure]) and bool(torch.isnan(xm[:, :, N:]).all())
    assert bool(torch.isfinite(part).all())
    terms = torch.stack((want.double(), want.double() * (x[:, :, :N].double() - mean.double()[:, None, None])), -1)   # [C][Lf][N][2]
    err = (part.double().sum(0) - terms.sum((1, 2))).abs()
    assert bool((err <= 1e-5 * terms.abs().sum((1, 2))).all()), (err, terms.abs().sum((1, 2)))


# ---------------------------------------------------------------------------------------------- unwritten padding
@pytest.mark.parametrize("name,shape", [("gru_bi", (300, 16, 128)), ("gru_uni", (33, 9, 64)), ("gru_uni", (528, 9, 64))],
                         ids=["gru_bi-300", "gru_uni-297", "gru_uni-S528"])
def test_blocks_read_no_memory_nobody_wrote(name, shape, monkeypatch):
    """engine.POISON_WORKSPACE fills every fresh workspace buffer that is not asked for as zero with NaN.  The stand-alone
    GRU blocks, forward and backward on fresh modules with the switch on and off: every output, gradient and BatchNorm
    buffer is finite and bit-identical between the two runs, so no kernel reads padding (frames >= N, sequences >= S)
    that nobody wrote.  gru_uni: 33 sequences of T = 9 (N = 297 frames, SP = 256), and 528 sequences (SP = 768)."""
    import tinyrecurrentunet_amd.engine as E
    from oracle import weights as W
    from tinyrecurrentunet_amd import network as hn
    args = {"gru_bi": (128, 64, 64, True), "gru_uni": (64, 128, 64, False)}[name]
    rng = np.random.default_rng(shape[0])
    x0 = torch.tensor(rng.standard_normal(shape) * 0.7, dtype=torch.float32)
    cot = torch.tensor(rng.standard_normal((shape[0], 64, shape[1])), dtype=torch.float32).cuda()

    def run(poison):
        monkeypatch.setattr(E, "POISON_WORKSPACE", poison)
        mod = W.fill_state_dict(hn.GRUBlock(*args), seed=13).cuda().train()
        x = x0.cuda().requires_grad_(True)
        y = mod(x)
        (y * cot).sum().backward()
        torch.cuda.synchronize()
        out = {"y": y.detach().clone(), "gx": x.grad.clone()}
        out.update({"g:" + n: p.grad.clone() for n, p in mod.named_parameters()})
        out.update({"buf:" + n: b.clone() for n, b in mod.named_buffers() if b.is_floating_point()})
        return out

    assert E.POISON_WORKSPACE is False
    on, off = run(True), run(False)
    assert set(on) == set(off) and len(on) >= 10
    for k in on:
        assert bool(torch.isfinite(on[k]).all()), "poisoned run: %s is not finite" % k
        assert bool(torch.isfinite(off[k]).all()), "plain run: %s is not finite" % k
    differ = [k for k in on if not torch.equal(on[k], off[k])]
    assert not differ, "tensors that depend on unwritten memory: %s" % differ
