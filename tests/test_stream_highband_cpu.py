"""No GPU: the float64 restatement of the stream pool's band above 8 kHz (tests/stream_highband_ref.py), the causality of
its gain, and the host plans of StreamPool(fs > 16 kHz, highband=) walked over every named rate."""
import os
import re

import numpy as np
import pytest
import torch

import stream_highband_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (22050, 24000, 32000, 44100, 48000, 88200, 96000)          # the named rates above 16 kHz
L16S = (257, 383, 384, 385)


def _sig(n, seed, scale=0.1):
    return scale * np.random.default_rng(seed).standard_normal(n)


# ---------------------------------------------------------------- the restatement
def test_restatement_fixed_points():
    lo = _sig(1000, 1)
    g, _ = SR.block_gains(np.zeros(1000), np.zeros(1000))
    assert g.shape == (8,) and (g == 1.0).all()                     # silence: (0 + eps) / (0 + eps)
    g, _ = SR.block_gains(lo, lo / 4)
    assert np.allclose(g[3:], 0.25, rtol=1e-7, atol=0) and np.allclose(g[:3], 0.25, rtol=1e-6, atol=0)
    g, _ = SR.block_gains(lo, np.zeros(1000), floor_db=-30.0)
    assert np.allclose(g, 10 ** -1.5, rtol=1e-12)
    g, _ = SR.block_gains(lo, 3 * lo)
    assert (g == 1.0).all()                                         # an enhancement that amplifies is capped
    G = SR.sample_gains(np.array([0.5, 1.0, 0.25]), 700, 1, 3)      # 48 kHz: D = 384 output samples per block
    assert G[0] == 0.5 and G[383] == 0.5                            # block 0 interpolates g_c[0] with itself
    assert G[384] == 0.5 and abs(G[384 + 192] - 0.75) < 1e-15       # block 1 walks from g_c[0] to g_c[1]


@pytest.mark.parametrize("fs", [48000, 44100])
def test_the_gain_is_causal(fs):
    import resample_ref as RR
    pd, qd = RR.ratio(fs, 16000)
    L16 = 1100
    L = (L16 - 1) * qd // pd + 1
    lo, ys = _sig(L16, 2), _sig(L16, 3, 0.03)
    g0, _ = SR.block_gains(lo, ys)
    G0 = SR.sample_gains(g0, L, pd, qd)
    jn, _, _ = SR.gain_index(np.arange(L), pd, qd)
    for j in (0, 3, 5, SR.n_blocks(L16) - 2):
        lo2, ys2 = lo.copy(), ys.copy()
        lo2[128 * (j + 1):] = _sig(L16 - 128 * (j + 1), 10 + j)
        ys2[128 * (j + 1):] *= -7.0
        g1, _ = SR.block_gains(lo2, ys2)
        assert (g1[:j + 1] == g0[:j + 1]).all() and not (g1[j + 1:] == g0[j + 1:]).all()
        G1 = SR.sample_gains(g1, L, pd, qd)
        assert (G1[jn <= j] == G0[jn <= j]).all()


# ---------------------------------------------------------------- the host plans
def _host_pool(slots, fs, highband="drop"):
    from tinyrecurrentunet_amd import streaming as sm
    pool = sm.StreamPool.__new__(sm.StreamPool)
    pool._host_init(slots, fs, torch.device("cuda"), highband)
    return pool


def _advance(pool, ids, pd, p16, pu, ph, closing=False):
    """what the device side of a call leaves in the host counters"""
    pool._down._recv[ids], pool._down._emit[ids] = pd.received, pd.emitted
    pool._hops[ids], pool._pend[ids] = (0, 0) if closing else (p16.hops, p16.pending)
    pool._up._recv[ids], pool._up._emit[ids] = pu.received, pu.emitted
    if ph is not None:
        hb = pool._hb
        hb._xc[ids], hb._lc[ids], hb._blk[ids] = ph.x_count, ph.lo_count, ph.blocks
        hb.up_lo._recv[ids], hb.up_lo._emit[ids] = pu.received, pu.emitted


def _cuts(L, how):
    if how == "all":
        return [L]
    if how == "empties":
        return [0, 7, 0, 0, L - 7, 0]
    return [how] * (L // how) + ([L % how] if L % how else [])


def _walk(fs, L16, how):
    """one session of the shortest length with L16 samples at 16 kHz, cut as ``how`` says, through the host plans of a
    "follow" pool and a "drop" pool side by side -> the largest occupancies seen"""
    pool, drop = _host_pool(2, fs, "follow"), _host_pool(2, fs)
    hb = pool._hb
    pdn, qdn = hb.pd, hb.qd
    L = (L16 - 1) * qdn // pdn + 1
    assert -(-L * pdn // qdn) == L16 and -(-(L - 1) * pdn // qdn) < L16
    ids = np.array(pool._alloc.open(2)[1:])                          # slot 1: the table carries the slot, not its position
    assert drop._alloc.open(2)[1] == ids[0]
    D = 128 * qdn
    most_x = most_lo = total = 0

    def check_gain_entries(ph, e0, count):
        """every output of the call finds its two block gains among [the slot's last two | the call's new blocks]"""
        if not count:
            return
        b0, bn = int(ph.table[0, 12]), int(ph.table[0, 13])
        n = np.arange(e0, e0 + count, dtype=np.int64)
        j = n * pdn // D
        assert j.max() <= b0 + bn - 1, (fs, L16, how, int(j.max()), b0, bn)         # block j is complete when n is emitted
        assert np.maximum(j - 1, 0).min() >= max(b0 - 2, 0), (fs, L16, how)

    for n in _cuts(L, how):
        lens = np.array([n], dtype=np.int64)
        e0 = int(pool._up._emit[ids][0])
        pd, p16, pu, ph = pool._plan_feed_at(lens, ids)
        dd, d16, du, dh = drop._plan_feed_at(lens, ids)
        assert dh is None and ph.out_lengths == pu.lengths == du.lengths             # feed returns what "drop" returns
        assert ph.n_paired == sum(p16.lengths) and ph.n_up == pu.n_out
        check_gain_entries(ph, e0, ph.out_lengths[0])
        _advance(pool, ids, pd, p16, pu, ph)
        _advance(drop, ids, dd, d16, du, None)
        assert hb._xc[ids][0] == pool._down._recv[ids][0] - pool._up._emit[ids][0]  # fed and not yet returned
        assert hb._lc[ids][0] == 128 * pool._hops[ids][0] + pool._pend[ids][0] - pool._up._recv[ids][0]
        most_x, most_lo = max(most_x, int(hb._xc[ids][0])), max(most_lo, int(hb._lc[ids][0]))
        total += ph.out_lengths[0]
    e0 = int(pool._up._emit[ids][0])
    pd, p16, pc, pu, ph, owed = pool._plan_close_at(ids)
    dd, d16, dc, du, dh, dowed = drop._plan_close_at(ids)
    assert ph.out_lengths == owed.tolist() == dowed.tolist() and total + ph.out_lengths[0] == L
    assert int(ph.table[0, 12]) + int(ph.table[0, 13]) == SR.n_blocks(L16)          # J blocks in all, the last may be partial
    check_gain_entries(ph, e0, ph.out_lengths[0])
    _advance(pool, ids, pd, p16, pu, ph, True)
    assert not hb._xc.any() and not hb._lc.any() and not hb._blk.any()
    assert most_x <= hb.xcap <= 4096 and most_lo <= 511
    return most_x, most_lo


@pytest.mark.parametrize("fs", RATES)
def test_plans_keep_their_bounds_and_the_counts_of_drop(fs):
    from tinyrecurrentunet_amd import stream_highband as SH
    worst = (0, 0)
    for L16 in L16S:
        for how in (160, 441, 960, "all", "empties") + ((1,) if L16 in (257, 385) else ()):
            worst = tuple(max(a, b) for a, b in zip(worst, _walk(fs, L16, how)))
    if fs in (44100, 48000):                                        # long enough, in single samples, to fill the lo line
        worst = tuple(max(a, b) for a, b in zip(worst, _walk(fs, 1043, 1)))
        assert worst[1] == 511
    pool = _host_pool(1, fs, "keep")
    assert pool._hb.xcap == SH.x_line_bound(pool._hb.pd, pool._hb.qd) == 543 * pool._hb.qd // pool._hb.pd
    print("%d Hz: x line %d of %d, lo line %d of 511" % (fs, worst[0], pool._hb.xcap, worst[1]))

def test_a_plan_that_would_pass_a_bound_is_refused():
    from tinyrecurrentunet_amd import stream_highband as SH
    ok = dict(slots=[0], x_count=[10], lo_count=[100], blocks=[0], emitted=[0], packet_lens=[960], x16_lens=[320],
              pair_lens=[128], up_off=[0], out_lens=[300], n_up=300, closing=False, xcap=1629)
    plan = SH.plan_highband(**ok)
    assert plan.x_count.tolist() == [670] and plan.lo_count.tolist() == [292] and plan.blocks.tolist() == [1] and plan.moves
    for bad in (dict(out_lens=[971]), dict(pair_lens=[512]), dict(pair_lens=[100]), dict(packet_lens=[2000]),
                dict(lo_count=[400]), dict(closing=True)):
        with pytest.raises(AssertionError):
            SH.plan_highband(**dict(ok, **bad))


# ---------------------------------------------------------------- arguments
def test_arguments_are_validated_without_a_device():
    from tinyrecurrentunet_amd import highband as HB
    from tinyrecurrentunet_amd import streaming as sm
    from tinyrecurrentunet_amd import stream_highband as SH
    for kw in (dict(highband="loud"), dict(highband=None), dict(highband_floor_db=0.5),
               dict(highband_floor_db=float("-inf")), dict(highband_floor_db=float("nan")), dict(highband_floor_db="3")):
        with pytest.raises(ValueError):
            sm.StreamPool(None, 1, fs=48000, **kw)                  # raised before the network is looked at
        with pytest.raises(ValueError):
            sm.StreamPool(None, 1, **kw)                            # ... at 16 kHz too
    with pytest.raises(TypeError):
        sm.StreamPool(None, 1, None, 0.5, False, 48000, "keep")    # keyword-only
    for fs in (16000, 8000, 12000):
        pool = _host_pool(2, fs, "follow")                          # validated, and then the pool of "drop"
        assert pool._hb is None and pool.highband == "follow" and pool.highband_floor_db == -30.0
    assert _host_pool(2, 48000)._hb is None and _host_pool(2, 48000).highband == "drop"
    pool = _host_pool(2, 48000, "keep")
    assert pool._hb.mode == "keep" and pool._hb._state is None      # no device buffer before the first launch
    assert SH.x_line_bound(1, 6) == 3258 and SH.x_line_bound(160, 441) == 1496
    with pytest.raises(ValueError, match="line"):
        SH.StreamHighband(128000, 1, "keep", -30.0, "cuda")         # 8 x 543 samples: a bound the buffer does not cover
    assert HB.MODES == ("drop", "keep", "follow")


def test_header_constants_match_the_module():
    from tinyrecurrentunet_amd import stream_highband as SH
    hdr = open(os.path.join(ROOT, "include", "trunet_hip.h")).read()
    val = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))
    assert (val("TRUNET_SHB_INTS"), val("TRUNET_SHB_LO_LINE"), val("TRUNET_SHB_MAX_X_LINE"), val("TRUNET_SHB_TILE")) == \
        (SH.INTS, SH.LO_LINE, SH.MAX_X_LINE, SH.TILE)
    assert SH.LO_BOUND < SH.LO_LINE and SH.HALO == val("TRUNET_HB_TAPS") - 1


def test_entry_points_reject_what_the_host_can_see():
    """TRUNET_EINVAL on the host, no launch: the pointers are never followed"""
    from tinyrecurrentunet_amd import _lib
    lib, E = _lib.lib(), _lib.TRUNET_EINVAL
    P = 4096                                                        # any non-null address
    ext = dict(n_sess=1, slots=1, xcap=1629, n_packet=960, n_up=960, n_x16=320, n_paired=256, n_blocks=2)

    def pair(lo_line=P, x16=P, paired=P, plan=P, tiles=1, **kw):
        e = dict(ext, **kw)
        return lib.trunet_stream_highband_pair(lo_line, x16, paired, plan, *e.values(), tiles, None)

    def join(up_y=P, x_line=P, out=P, plan=P, g=P, tiles=1, pd=1, qd=3, mode=2, **kw):
        e = dict(ext, **kw)
        return lib.trunet_stream_highband_join(up_y, P, x_line, P, g, out, plan, *e.values(), tiles, pd, qd, mode, None)

    def gains(halo=P, eline=P, plan=P, g_min=0.03, **kw):
        e = dict(ext, **kw)
        return lib.trunet_stream_highband_gains(P, P, halo, P, P, P, eline, P, plan, *e.values(), g_min, None)

    def commit(x_line=P, lo_line=P, plan=P, halo=P, mode=2, **kw):
        e = dict(ext, **kw)
        return lib.trunet_stream_highband_commit(x_line, P, lo_line, P, halo, P, P, P, P, P, P, plan, *e.values(), mode, None)

    for kw in (dict(lo_line=None), dict(x16=None), dict(paired=None), dict(plan=None), dict(n_sess=0), dict(slots=0),
               dict(xcap=0), dict(xcap=4097), dict(n_paired=-1), dict(n_blocks=1), dict(n_blocks=3), dict(tiles=2),
               dict(tiles=-1), dict(n_x16=2 ** 31)):
        assert pair(**kw) == E, kw
    for kw in (dict(up_y=None), dict(x_line=None), dict(out=None), dict(plan=None), dict(g=None), dict(tiles=2), dict(pd=0),
               dict(pd=3), dict(qd=641), dict(mode=0), dict(mode=3), dict(n_up=-1), dict(n_sess=0)):
        assert join(**kw) == E, kw
    for kw in (dict(halo=None), dict(eline=None), dict(plan=None), dict(g_min=0.0), dict(g_min=1.5), dict(g_min=float("nan")),
               dict(n_blocks=5), dict(slots=0)):
        assert gains(**kw) == E, kw
    for kw in (dict(x_line=None), dict(lo_line=None), dict(plan=None), dict(halo=None), dict(mode=0), dict(n_packet=-1),
               dict(xcap=5000)):
        assert commit(**kw) == E, kw
