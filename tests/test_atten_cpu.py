"""The attenuation limit (tinyrecurrentunet_amd/atten.py) without a GPU: the gain of a limit, every refusal
before anything reaches the device, the host plan of the pool's launch, the entry points' own refusals, the command line, and
the restatement's ramp (tests/atten_ref.py)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import atten_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
BAD = [-1.0, -1e-9, float("nan"), -INF, True, False, np.bool_(True), "12", 1 + 0j]


def _net(**kw):
    from tinyrecurrentunet_amd.network import TRUNet
    return TRUNet(input_size=4, **kw).eval()


def _host_pool(slots, atten_lim_db, fs=16000):
    """the host side of a StreamPool: everything its checks need, and no device"""
    from tinyrecurrentunet_amd import streaming as sm
    pool = sm.StreamPool.__new__(sm.StreamPool)
    pool._host_init(slots, fs, torch.device("cuda"), "drop", -30.0, atten_lim_db)
    return pool


# ---------------------------------------------------------------- 1. L -> g
def test_gain_of_a_limit():
    from tinyrecurrentunet_amd import atten as AT
    assert AT.gain(0) == np.float32(1.0) and AT.gain(0.0).dtype == np.float32
    assert AT.gain(INF) == np.float32(0.0)
    for L in (1e-3, 3, 6.0, 12, 20.0, 40, 99.5, np.float32(6.0), np.int64(12)):
        want = np.float32(10.0 ** (-float(L) / 20.0))                 # float64 on the host, one rounding to fp32
        assert AT.gain(L) == want and AT.gain(L) == np.float32(AR.gain(float(L))), L
    assert AT.gain(20.0) == np.float32(0.1) and abs(float(AT.gain(6.0)) - 0.5011872336) < 3e-8
    assert AT.gain(2000.0) == 0.0                                     # below the smallest fp32: no limit
    g = AT.gains([0, 6.0, INF], 3)
    assert g.dtype == np.float32 and g.tolist() == [1.0, float(AT.gain(6.0)), 0.0]
    assert AT.gains(12.0, 4).tolist() == [float(AT.gain(12.0))] * 4
    assert AT.gains(torch.tensor([0.0, 20.0]), 2).tolist() == [1.0, float(np.float32(0.1))]
    assert AT.gains(np.array([40, 0]), 2).tolist() == [float(np.float32(0.01)), 1.0]
    assert AT.gains([], 0).shape == (0,)


# ---------------------------------------------------------------- 2. refusals, all before the device
@pytest.mark.parametrize("bad", BAD, ids=[repr(b) for b in BAD])
def test_gain_refuses(bad):
    from tinyrecurrentunet_amd import atten as AT
    with pytest.raises(ValueError, match="atten_lim_db"):
        AT.gain(bad)
    with pytest.raises(ValueError, match="atten_lim_db"):
        AT.gains([6.0, bad], 2)


def test_gains_refuse_a_wrong_length_and_bool_arrays():
    from tinyrecurrentunet_amd import atten as AT
    with pytest.raises(ValueError, match="atten_lim_db"):
        AT.gain(None)
    for v, n in (([6.0, 12.0], 3), ([6.0], 0), ((1, 2, 3), 2), (torch.tensor([1.0, 2.0]), 1), (np.zeros(4), 5)):
        with pytest.raises(ValueError, match="values for"):
            AT.gains(v, n)
    for v in (torch.tensor([True, False]), np.array([True, False]), [True, 6.0]):
        with pytest.raises(ValueError, match="atten_lim_db"):
            AT.gains(v, 2)


def test_enhance_refuses_before_anything_reaches_the_device():
    from tinyrecurrentunet_amd.enhance import enhance
    net = _net()
    ok = torch.zeros(1000)                                            # CPU tensors: reaching the device check is a TrunetHipError
    for fs in (16000, 48000):
        for bad in (-3.0, float("nan"), True, [6.0, -1.0], [6.0], [6.0, 12.0, 20.0], torch.tensor([True, False])):
            with pytest.raises(ValueError, match="atten_lim_db"):
                enhance(net, [ok, ok], fs=fs, atten_lim_db=bad)
    assert enhance(net, [], atten_lim_db=6.0) == [] and enhance(net, [], atten_lim_db=[]) == []


def test_streams_and_pools_refuse_before_anything_reaches_the_device():
    from tinyrecurrentunet_amd import _lib
    from tinyrecurrentunet_amd.streaming import AudioStream, StreamPool
    net = _net()                                                      # on the CPU: past the checks waits a TrunetHipError
    for bad in (-3.0, float("nan"), True, [6.0, -1.0], [6.0]):
        with pytest.raises(ValueError, match="atten_lim_db"):
            AudioStream(net, 2, atten_lim_db=bad)
    for bad in (-3.0, float("nan"), True, [6.0, 6.0]):                # a pool opens every session with ONE limit
        with pytest.raises(ValueError, match="atten_lim_db"):
            StreamPool(net, 2, atten_lim_db=bad)
    with pytest.raises(_lib.TrunetHipError):
        AudioStream(net, 2, atten_lim_db=[6.0, INF])
    with pytest.raises(_lib.TrunetHipError):
        StreamPool(net, 2, atten_lim_db=INF)


def test_set_atten_lim_refusals_change_nothing():
    plain = _host_pool(4, None)
    ids = plain.open(2)
    assert plain.atten_lim_db is None and plain._g_tgt is None
    with pytest.raises(ValueError, match="built without atten_lim_db"):
        plain.set_atten_lim(ids, 6.0)
    pool = _host_pool(4, 12.0)
    g12 = np.float32(10.0 ** (-12.0 / 20.0))
    assert pool.atten_lim_db == 12.0 and pool._g_tgt.dtype == np.float32 and (pool._g_tgt == g12).all()
    a, b = pool.open(2)
    before = pool._g_tgt.copy()
    for bad_ids in ([a, 3], [a, a], [7], [-1], torch.tensor([2])):    # idle, listed twice, outside the pool
        with pytest.raises(ValueError, match="slot"):
            pool.set_atten_lim(bad_ids, 6.0)
    for bad in (-1.0, float("nan"), True, [6.0], [6.0, 6.0, 6.0], [6.0, -2.0], "6"):
        with pytest.raises(ValueError, match="atten_lim_db"):
            pool.set_atten_lim([a, b], bad)
    assert (pool._g_tgt == before).all()
    pool.set_atten_lim([], 6.0)                                       # nothing listed: nothing to do, no device
    pool._g_tgt[a] = 0.25                                             # what a live change leaves ...
    pool.abort([a])
    assert pool.open(1) == [a] and pool._g_tgt[a] == g12 and pool._g_stale      # ... does not reach the slot's next session


def test_plan_atten():
    from tinyrecurrentunet_amd import atten as AT
    tab, keep = AT.plan_atten([5, 2, 7], [384, 200, 0], [0, 128, 256], [128, 128, 0], [0, 128, 256], [128, 0, 0],
                              [False, True, False], False)
    assert tab.dtype == np.int32 and tab.shape == (3, AT.INTS) and keep.tolist() == [384, 328, 0]
    assert tab.tolist() == [[5, 384, 0, 128, 0, 128, 0, 0], [2, 200, 128, 128, 0, 0, AT.FIRST, 0], [7, 0, 0, 0, 0, 0, 0, 0]]
    tab, keep = AT.plan_atten([1], [447], [0], [0], [512], [447], [False], True)
    assert tab.tolist() == [[1, 447, 0, 0, 512, 447, AT.CLOSING, 0]] and keep.tolist() == [0]
    with pytest.raises(AssertionError):
        AT.plan_atten([1], [100], [0], [28], [0], [129], [False], False)           # gives more than it holds
    with pytest.raises(AssertionError):
        AT.plan_atten([1], [384], [0], [128], [0], [0], [False], False)            # would keep 512
    with pytest.raises(AssertionError):
        AT.plan_atten([1], [384], [0], [1], [0], [384], [False], True)             # a closing session leaves a sample
    with pytest.raises(ValueError):
        AT.plan_atten([1, 2], [384], [0], [1], [0], [384], [False], False)
    assert (AT.INTS, AT.DRY_LINE, AT.FIRST, AT.CLOSING, AT.DRY_BOUND) == (8, 512, 1, 2, 511)


def test_the_header_carries_the_constants_of_the_host_plan():
    import re
    from tinyrecurrentunet_amd import atten as AT
    text = open(os.path.join(ROOT, "include", "trunet_hip.h")).read()
    val = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    assert (val("TRUNET_ATT_INTS"), val("TRUNET_ATT_DRY_LINE"), val("TRUNET_ATT_FIRST"), val("TRUNET_ATT_CLOSING")) == \
           (AT.INTS, AT.DRY_LINE, AT.FIRST, AT.CLOSING)


def test_entry_points_refuse_what_the_host_can_see():
    from tinyrecurrentunet_amd import _lib
    lib, E = _lib.lib(), _lib.TRUNET_EINVAL
    a, d, g, so, pl = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    rag = lib.trunet_atten_blend_ragged
    for args in ((None, d, g, so, 1, 1000), (a, None, g, so, 1, 1000), (a, d, None, so, 1, 1000), (a, d, g, None, 1, 1000),
                 (a, d, g, so, 0, 1000), (a, d, g, so, -2, 1000), (a, d, g, so, 1, 256), (a, d, g, so, 4, 1000)):
        assert rag(*args, None) == E, args
    rows = lib.trunet_atten_blend_rows
    for args in ((None, d, g, 2, 128, 128, 512), (a, None, g, 2, 128, 128, 512), (a, d, None, 2, 128, 128, 512),
                 (a, d, g, 0, 128, 128, 512), (a, d, g, 2, 0, 128, 512), (a, d, g, 2, 128, 127, 512),
                 (a, d, g, 2, 128, 128, 127), (a, d, g, 2 ** 24, 128, 128, 512)):
        assert rows(*args, None) == E, args
    pool = lib.trunet_stream_atten
    gc, gt, pk = 0x6000, 0x7000, 0x8000
    for args in ((a, None, gc, gt, pk, pl, 2, 8, 256, 256), (a, d, None, gt, pk, pl, 2, 8, 256, 256),
                 (a, d, gc, None, pk, pl, 2, 8, 256, 256), (a, d, gc, gt, pk, None, 2, 8, 256, 256),
                 (a, d, gc, gt, pk, pl, 0, 8, 256, 256), (a, d, gc, gt, pk, pl, 2, 0, 256, 256),
                 (a, d, gc, gt, pk, pl, 2, 8, -1, 256), (a, d, gc, gt, pk, pl, 2, 8, 256, -1),
                 (a, d, gc, gt, None, pl, 2, 8, 256, 256), (None, d, gc, gt, pk, pl, 2, 8, 256, 256)):
        assert pool(*args, None) == E, args


# ---------------------------------------------------------------- 3. the command line
def test_the_command_line_parses_the_limit():
    run = lambda *a: subprocess.run([sys.executable, "-m", "tinyrecurrentunet_amd.enhance", *a], cwd=ROOT,
                                    capture_output=True, text=True, timeout=120)
    r = run("--help")
    assert r.returncode == 0 and "--atten-lim-db" in r.stdout, r.stderr
    base = ("--checkpoint", "none.pt", "--input-size", "4", "--in", "no_such_dir_in", "--out", "no_such_dir_out")
    for bad in ("-3", "nan", "twelve"):
        r = run(*base, "--atten-lim-db", bad)
        assert r.returncode == 2 and "atten" in r.stderr, (bad, r.returncode, r.stderr)
    for good in ("12", "0", "inf"):                                   # parsed and accepted: the run gets as far as the folder
        r = run(*base, "--atten-lim-db", good)
        assert r.returncode not in (0, 2) and "no_such_dir_in" in r.stderr, (good, r.returncode, r.stderr)


# ---------------------------------------------------------------- 4. the restatement's ramp
def test_the_ramp_is_continuous_and_lands_on_the_new_gain():
    for g_old, g_new in ((1.0, 0.1), (0.1, 1.0), (AR.gain(6.0), 0.0), (0.0, AR.gain(40.0)), (0.25, 0.25)):
        r = AR.ramp(g_old, g_new)
        step = abs(g_new - g_old) / 128
        assert r.shape == (128,) and r[-1] == g_new
        assert abs(r[0] - g_old) <= step * (1 + 1e-12)                # across the boundary to the hop before ...
        assert np.all(np.abs(np.diff(r)) <= step * (1 + 1e-9) + 1e-18)        # ... inside, and so to the hop after (r[-1] = g_new)
        assert np.all(np.diff(r) * (g_new - g_old) >= 0)              # monotone
    g, in_ramp = AR.session_gains(1600, 0.1, [(700, 0.5)])            # fed 5 hops and 60 samples: two hops are out
    assert np.all(g[:256] == 0.1) and not in_ramp[:256].any() and in_ramp[256:384].all() and not in_ramp[384:].any()
    assert np.all(g[256:384] == AR.ramp(0.1, 0.5)) and np.all(g[383:] == 0.5)
    assert abs(g[256] - g[255]) <= 0.4 / 128 * (1 + 1e-12)
    for P in (700, 701, 767):                                         # the ramp's place follows the samples fed, in whole hops
        assert np.array_equal(AR.session_gains(1600, 0.1, [(P, 0.5)])[0], AR.session_gains(1600, 0.1, [(640, 0.5)])[0])
    g, in_ramp = AR.session_gains(1000, 0.1, [(383, 0.5)])            # before frame 0: the session starts at the new gain
    assert np.all(g == 0.5) and not in_ramp.any()
    g, in_ramp = AR.session_gains(1000, 0.1, [(384, 0.5), (896, 0.0)])
    assert np.all(g[:128] == AR.ramp(0.1, 0.5)) and np.all(g[128:512] == 0.5) and np.all(g[512:640] == AR.ramp(0.5, 0.0))
    assert np.all(g[639:] == 0.0) and in_ramp.sum() == 256
    x, y = np.array([1.0, -2.0, 0.5]), np.array([0.5, 1.0, 0.5])
    assert np.array_equal(AR.blend(x, y, 0.0), y) and np.array_equal(AR.blend(x, y, 1.0), x)
    assert np.array_equal(AR.bound(x, y), 4 * 2.0 ** -24 * np.array([1.5, 3.0, 1.0]))
    assert math.isclose(AR.gain(20.0), 0.1, rel_tol=1e-7) and AR.gain(float("inf")) == 0.0 and AR.gain(0.0) == 1.0


# ---------------------------------------------------------------- the pool's host plans, walked with the kernel's restatement
def _walk(slots, sessions, seed):
    """Sessions (samples, "feed" or "step", gain, changes [(P, gain)]) through the HOST side of a pool with a limit, every
    call's blend stage carried out by atten_ref.stream_atten on x[p] = p + 1 and a wet signal of zeros, so that a session's
    output divided by x is the gain each sample was given, and exactly so where the gain is a power of two.  Random packets
    (empty ones too), random pauses, slots used again.  -> per session (gains, largest dry-line occupancy)."""
    from tinyrecurrentunet_amd import streaming as sm
    rng = np.random.default_rng(seed)
    pool = _host_pool(slots, 0.0)
    S, HOP = slots, 128
    dry, g_cur, g_tgt = np.full((S, AR.LINE), np.nan), np.full(S, np.nan), np.full(S, np.nan)
    xs = [np.arange(1, n + 1, dtype=np.float64) for n, _, _, _ in sessions]
    todo, slot, at, got, peak = list(range(len(sessions))), {}, {}, {i: [] for i in range(len(sessions))}, {}

    def targets():
        g_tgt[:] = pool._g_tgt                                        # what _push_targets copies

    def moves(i):
        for P, g in sessions[i][3]:
            if P == at[i]:
                pool._g_tgt[slot[i]] = g                              # what set_atten_lim leaves on the host

    while todo or slot:
        while todo and pool.free:
            i = todo.pop(0)
            (slot[i],) = pool.open(1)
            at[i], peak[i] = 0, 0
            pool._g_tgt[slot[i]] = sessions[i][2]
        for i in slot:
            moves(i)
        targets()
        live = [i for i in sorted(slot) if rng.random() < 0.8]
        feeds = [i for i in live if sessions[i][1] == "feed" and at[i] < len(xs[i])]
        if feeds:
            ids = np.array([slot[i] for i in feeds])
            lens = []
            for i in feeds:
                stop = min([P for P, _ in sessions[i][3] if P > at[i]] + [len(xs[i])])      # a call never straddles a change
                lens.append(int(min(rng.choice([0, 1, 127, 128, 129, 160, 1000]), stop - at[i])))
            plan = sm.plan_feed(pool._hops, pool._pend, np.array(lens), ids)
            att = pool._att_feed(plan)
            packet = np.concatenate([xs[i][at[i]:at[i] + m] for i, m in zip(feeds, lens)])
            out = np.zeros(plan.n_out * HOP)
            if att is not None:
                assert AR.stream_atten(att, out, dry, g_cur, g_tgt, packet) == list(range(len(feeds)))
            pool._hops[ids], pool._pend[ids] = plan.hops, plan.pending
            for i, m, o, k in zip(feeds, lens, plan.out_off, plan.lengths):
                got[i].append(out[HOP * int(o):HOP * int(o) + k])
                at[i] += m
        steps = [i for i in live if sessions[i][1] == "step" and at[i] + HOP <= len(xs[i])]
        if steps:
            ids = np.array([slot[i] for i in steps])
            plan = sm.plan_step(pool._hops, ids)
            att = pool._att_step(ids, plan)
            chunks = np.concatenate([xs[i][at[i]:at[i] + HOP] for i in steps])
            out = np.zeros(len(steps) * HOP)
            assert AR.stream_atten(att, out, dry, g_cur, g_tgt, chunks) == list(range(len(steps)))
            pool._hops[ids] = plan.hops
            for k, i in enumerate(steps):
                if plan.valid[k]:
                    got[i].append(out[HOP * k:HOP * (k + 1)])
                at[i] += HOP
        for i in slot:
            peak[i] = max(peak[i], int(pool._dry_count(np.array([slot[i]]))[0]))
            moves(i)
        targets()
        done = [i for i in live if len(xs[i]) - at[i] < (HOP if sessions[i][1] == "step" else 1)]
        if done:
            ids = np.array([slot[i] for i in done])
            tails = [xs[i][at[i]:] if sessions[i][1] == "step" else None for i in done]
            rs = [int(pool._pend[slot[i]]) if t is None else len(t) for i, t in zip(done, tails)]
            plan = sm.plan_close(pool._hops[ids], rs, ids)
            att = pool._att_close(ids, plan, tails, rs)
            tl = np.zeros((len(done), HOP))
            for k, t in enumerate(tails):
                if t is not None:
                    tl[k, :len(t)] = t
            out = np.zeros(len(done) * sm.CLOSE_OUT_ROWS * HOP)
            assert AR.stream_atten(att, out, dry, g_cur, g_tgt, tl.reshape(-1)) == list(range(len(done)))
            pool._alloc.release(ids)
            for k, (i, m) in enumerate(zip(done, plan.lengths)):
                got[i].append(out[sm.CLOSE_OUT_ROWS * HOP * k:sm.CLOSE_OUT_ROWS * HOP * k + m])
                del slot[i]
    return [(np.concatenate(got[i]) / xs[i], peak[i]) for i in range(len(sessions))]


def test_the_pools_plans_pair_every_output_with_its_own_dry_sample():
    """gain 1 everywhere: the output IS the dry line, so out[p] = x[p] exactly says that every output sample was paired with
    the input sample at its own position, whatever the packets, pauses and slots were"""
    sessions = [(n, how, 1.0, []) for n in (257, 383, 384, 385, 1152, 4000, 513, 2 * 128 + 64, 9 * 128 + 127)
                for how in ("feed", "step")]
    for seed in range(3):
        res = _walk(4, sessions, seed)
        for (n, how, _, _), (g, peak) in zip(sessions, res):
            assert g.shape == (n,) and np.all(g == 1.0), (n, how, seed)
            assert peak <= 511
        assert max(peak for _, peak in res) == 511                    # the line's bound is reached


def test_the_pools_plans_put_the_ramp_where_the_samples_fed_say():
    """gains that are powers of two: the restated kernel's gain per sample against atten_ref.session_gains, exactly"""
    sessions = [(1600, "feed", 0.25, [(700, 1.0)]), (1600, "step", 0.25, [(768, 1.0)]), (1600, "feed", 0.5, [(256, 0.125)]),
                (1000, "feed", 1.0, [(384, 0.5), (896, 0.0)]), (1279, "step", 0.5, [(384, 0.25), (1152, 1.0)]),
                (1600, "feed", 0.25, [(1600, 1.0)]), (320, "step", 0.5, [(256, 1.0)]), (400, "feed", 1.0, []),
                (900, "feed", 0.5, [(383, 0.25)]), (900, "feed", 0.5, [(511, 0.25)])]
    for seed in range(3):
        for (n, how, g0, changes), (g, _) in zip(sessions, _walk(3, sessions, seed)):
            want, _ = AR.session_gains(n, g0, changes)
            assert np.array_equal(g, want), (n, how, changes, seed, int(np.argmax(g != want)))
