"""The bf16-octet recurrence kernels of bf16_gru.hip (trunet_bf16_gru_fwd / _bwd, both TRUNET_GRU_NE instances), each on its
own through the C ABI against the fp64 restatement of tests/gru_ref.py.  The comparison is bgru_ref.inside: every stored
element lies between rne_bf16(fp64 - B) and rne_bf16(fp64 + B), B being the bound the fp32 pin allows gru.hip on the same
inputs -- an interval with no tolerance of its own, measured from the references and never from the kernel
(tests/test_bgru_ref_cpu.py shows what it rejects).  Every output is prefilled with NaN and has one more octet behind it,
which must stay NaN; every input must hold the same bits after the launch (bgru_cases._launched)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import bgru_cases as C
import bgru_ref as B
import gru_cases as G

pytestmark = pytest.mark.gpu
ROOT = C.ROOT
H = B.H


def _id(case):
    return "-".join(str(v) for v in case)


@pytest.fixture(scope="module", params=C.CASES, ids=_id)
def bgru(request):
    """inputs and the fp64 / fp32 forward references of one case, computed once and shared by the tests below (never
    modified)"""
    return C.case(*request.param)


def test_bgru_forward(bgru):
    C.check_fwd(bgru)


def test_bgru_backward_on_the_reference_state(bgru):
    C.check_bwd(bgru, own=False)


def test_bgru_backward_on_the_forward_kernels_outputs(bgru):
    C.check_bwd(bgru, own=True)


@pytest.mark.parametrize("L,NP", [(16, 384), (17, 128)])
def test_bgru_backward_gradient_that_exists_only_through_the_carry(L, NP):
    """dhout is non-zero at a single position, the last one each direction visits: every dgi at the other positions is
    W_hh^T dgh and dh z carried back, nothing else"""
    c = C.case("long", L, NP)
    dh = torch.zeros_like(c.dhout)
    dh[:H, L - 1] = c.dhout[:H, L - 1]
    dh[H:, 0] = c.dhout[H:, 0]
    _, _, r64 = C.check_bwd(c, own=False, dhout=dh, what="bwd(carry only)")
    assert float(r64[0][:3 * H, 0].abs().max()) > 0 and float(r64[0][3 * H:, L - 1].abs().max()) > 0


def _all(gi, whh, bhh, dhout):
    hout, gates = C.gpu_bgru_fwd(gi, whh, bhh)
    dgi, dghn = C.gpu_bgru_bwd(dhout, (hout, gates), whh)
    return {"hout": hout, "gates": gates, "dgi": dgi, "dghn": dghn}


def test_bgru_columns_are_independent():
    """Column n of every output, forward and backward, is bit for bit the same whether the other columns hold zeros, the
    overflow regime or NaN octets (the kernels take no N: a padded frame carries whatever the projection left there), and
    whether the column sits in an NP = 128 or (at another lane and workgroup) an NP = 512 launch"""
    L = 16
    c = C.inputs("ordinary", L, 128)
    o = C.inputs("overflow", L, 512)
    base = _all(c.gi, c.whh, c.bhh, c.dhout)
    keep = torch.arange(128) % 3 == 0

    def embed(t, other, off, NP):
        out = other[..., :NP].clone()
        out[..., off:off + 128][..., keep] = t[..., keep]
        return out

    zero = lambda t: torch.zeros(t.shape[:-1] + (512,))
    nan = lambda t: torch.full(t.shape[:-1] + (512,), float("nan"))
    over = lambda t: o.gi if t.shape[0] == 6 * H else B.rne(o.dhout * 200.0)
    for name, (other, off, NP) in {"zeros": (zero, 0, 128), "overflow": (over, 0, 128), "NaN": (nan, 0, 128),
                                   "NP512": (zero, 200, 512), "NP512+overflow": (over, 200, 512),
                                   "NP512+NaN": (nan, 200, 512)}.items():
        got = _all(embed(c.gi, other(c.gi), off, NP), c.whh, c.bhh, embed(c.dhout, other(c.dhout), off, NP))
        for k, v in got.items():
            mine = v[..., off:off + 128][..., keep]
            assert bool(torch.isfinite(v if "NaN" not in name else mine).all()), (name, k)
            assert torch.equal(mine, base[k][..., keep]), (name, k)


def test_bgru_directions_are_independent():
    """zeroing one direction's W_hh and gi leaves the other direction's octets bit-identical"""
    c = C.inputs("trained", 16, 128)
    base = _all(c.gi, c.whh, c.bhh, c.dhout)
    for d in range(2):
        gi, whh = c.gi.clone(), c.whh.clone()
        gi[d * 3 * H:(d + 1) * 3 * H] = 0
        whh[d] = 0
        got = _all(gi, whh, c.bhh, c.dhout)
        k = 1 - d
        assert torch.equal(got["hout"][k * H:(k + 1) * H], base["hout"][k * H:(k + 1) * H])
        assert torch.equal(got["gates"][k], base["gates"][k])
        assert torch.equal(got["dgi"][k * 3 * H:(k + 1) * 3 * H], base["dgi"][k * 3 * H:(k + 1) * 3 * H])
        assert torch.equal(got["dghn"][k * H:(k + 1) * H], base["dghn"][k * H:(k + 1) * H])
        assert not torch.equal(got["hout"][d * H:(d + 1) * H], base["hout"][d * H:(d + 1) * H])


_IN_PROCESS = {}


@pytest.mark.parametrize("ne", ["1", "2"])
def test_bgru_both_kernel_instances_in_a_fresh_interpreter(ne, tmp_path):
    """TRUNET_GRU_NE = 1 / 2 forces bgru_fwd_kernel<NE> and bgru_bwd_kernel<NE> (the default runs <2> forward and <1>
    backward, so <1> forward and <2> backward are launched by nothing else).  bgru_ne() latches the environment at its
    first call: one child interpreter per value, one after the other, runs bgru_cases.CHILD_CASES against the same
    intervals and reports a checksum of every output tensor.  Both instances do the same operations per column in the
    same order, so the checksums must equal those of the in-process default."""
    out = str(tmp_path / "child.json")
    env = dict(os.environ, TRUNET_GRU_NE=ne)
    try:
        p = subprocess.run([sys.executable, "tests/bgru_cases.py", out], cwd=ROOT, env=env, timeout=180,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    except subprocess.TimeoutExpired as e:
        pytest.fail("TRUNET_GRU_NE=%s child timed out:\n%s" % (ne, e.output))
    assert p.returncode == 0, "TRUNET_GRU_NE=%s child ended with %d:\n%s" % (ne, p.returncode, p.stdout[-4000:])
    child = json.load(open(out))
    assert child["TRUNET_GRU_NE"] == ne and len(child["sums"]) == len(C.CHILD_CASES)
    if not _IN_PROCESS:
        _IN_PROCESS.update(C.run_cases())
    diff = [(c, k) for c, s in _IN_PROCESS["sums"].items() for k in s if child["sums"][c][k] != s[k]]
    assert not diff, "TRUNET_GRU_NE=%s differs from the in-process default in %s" % (ne, diff)


def test_bgru_stored_values_against_the_fp32_kernels_of_gru_hip():
    """Per tensor, the number of elements whose stored value differs from rne_bf16 of what trunet_gru_fwd / _bwd give in
    fp32 on the same operands (forward: the same gi; backward: the same dhout and the bf16 forward's own stored state).
    The two source texts do the same arithmetic per column, and on the MI355X hipcc contracts them alike: every count is
    zero (profiles/parity_bgru.txt), so equality is asserted.  (The one-ulp comparison of tests/test_bf16_gpu.py stays.)"""
    c = C.inputs("ordinary", 16, 384)
    got = _all(c.gi, c.whh, c.bhh, c.dhout)
    hout, gates = G.gpu_fgru_fwd(c.gi, c.whh, c.bhh)
    dgi, dghn = G.gpu_fgru_bwd(c.dhout, got["hout"], got["gates"], c.whh)
    ref = {"hout": hout, "gates": gates, "dgi": dgi, "dghn": dghn}
    counts = {k: (int((B.rne(ref[k]) != got[k]).sum()), got[k].numel()) for k in got}
    C.report("BGRU vs rne_bf16(gru.hip) ordinary L=16 NP=384: elements that differ  "
             + "  ".join("%s %d/%d" % ((k,) + counts[k]) for k in counts))
    assert all(n == 0 for n, _ in counts.values()), counts
