"""No GPU: the host side of the stateful resampler (tinyrecurrentunet_amd/resample.py: ready, history, plan_stream,
StreamResampler; streaming.py: StreamPool(fs=)) -- the float64 restatement of the stream against the
restatement of the whole, the planners against a row-by-row loop, and every refusal that needs no device."""
import numpy as np
import pytest
import torch

import resample_ref as RR
import stream_resample_ref as SR

RATIOS = [(1, 3), (3, 1), (160, 441), (441, 160), (2, 1), (1, 2), (1, 6), (640, 441)]


def _lengths(p, q):
    half = 16 * max(p, q)
    K = RR.taps_per_output(p, half)
    ahead = -(-half // p)                    # ready(N) > 0 from N = ahead + 1 on (N p > half)
    return sorted({1, 2, K - 2, K - 1, K, ahead - 1, ahead, ahead + 1, ahead + 2, 3001})


def _cuts(L, style, rng):
    if style == "singles":
        return list(range(1, L))
    if style == "empties":                   # every sample on its own, an empty packet before and after each
        return [i for i in range(0, L + 1) for _ in range(2)]
    if style in ("160", "441"):
        return list(range(int(style), L, int(style)))
    if style == "random":
        return sorted(rng.integers(0, L + 1, size=min(L, 12)).tolist())
    return []                                # one piece


@pytest.mark.parametrize("pq", RATIOS)
def test_the_stream_cut_anywhere_is_the_whole(pq):
    p, q = pq
    half = 16 * max(p, q)
    H = SR.history(p, half)
    rng = np.random.default_rng(1000 * p + q)
    for L in _lengths(p, q):
        x = rng.standard_normal(L)
        want, _ = RR.resample(x, p, q)
        M = -(-L * p // q)
        assert want.shape == (M,)
        for style in ("singles", "empties", "160", "441", "random", "one"):
            if L == 3001 and style == "empties":
                continue                     # "singles" covers the long session sample by sample
            feeds, rest, s = SR.run(x, _cuts(L, style, rng), p, q)
            got = np.concatenate(feeds + [rest])
            assert got.shape == (M,), (pq, L, style)
            assert sum(len(f) for f in feeds) + len(rest) == M
            assert np.max(np.abs(got - want), initial=0.0) <= 1e-12, (pq, L, style)
            assert sum(len(f) for f in feeds) == SR.ready(L, p, q, half)
            assert max(s.lowest, default=0) <= H, (pq, L, style, max(s.lowest), H)
            assert (s.N, s.E) == (0, 0)      # closed: the slot starts afresh


@pytest.mark.parametrize("pq", RATIOS)
def test_ready_and_history(pq):
    from tinyrecurrentunet_amd import resample as R
    p, q = pq
    h, half = R.design(p, q)
    K = R.taps_per_output(p, half)
    assert R.history(p, half) == K - 1 == SR.history(p, half)
    N = np.arange(0, 4 * K + 50)
    r = R.ready(N, p, q, half)
    assert r.tolist() == [SR.ready(int(n), p, q, half) for n in N] == [R.ready(int(n), p, q, half) for n in N]
    assert (np.diff(r) >= 0).all() and (r <= -(-N * p // q)).all()
    assert R.ready(0, p, q, half) == 0 and isinstance(R.ready(5, p, q, half), int)
    # ready(N) outputs read no sample at or past N, the next one does: m q + half < N p exactly for m < ready(N)
    for n in (1, K - 1, K, 3 * K + 7):
        m = R.ready(n, p, q, half)
        assert m == 0 or ((m - 1) * q + half) // p <= n - 1
        assert (m * q + half) // p >= n
        # ... and the lowest sample of output m is not below n - history
        assert (m * q + half) // p - (K - 1) >= n - R.history(p, half)
    # the look-ahead: half / p input samples, 16 at the lower of the two rates
    assert half / p == 16 * max(p, q) / p


def test_history_is_small_for_the_named_rates():
    from tinyrecurrentunet_amd import resample as R
    for fs in (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000):
        for a, b in ((fs, 16000), (16000, fs)):
            p, q = R.ratio(a, b)
            assert R.history(p, 16 * max(p, q)) < 200, (a, b)
    assert R.StreamResampler(16000, 25, 2).H == R.MAX_HISTORY     # 1/640, the longest history ratio() allows


def _loop_plan(received, emitted, lengths, closing, p, q, half, tile, slots):
    rows, poff, ooff, t = [], 0, 0, 0
    for N0, E0, n, c, s in zip(received, emitted, lengths, closing, slots):
        N1 = N0 + n
        target = -(-N1 * p // q) if c else SR.ready(N1, p, q, half)
        cnt = target - E0
        tiles = -(-cnt // tile)
        rows.append([s, N0, poff, n, E0, cnt, ooff, int(c), t, t + tiles])
        poff, ooff, t = poff + n, ooff + cnt, t + tiles
    return rows


def test_plan_stream_matches_a_row_by_row_loop():
    from tinyrecurrentunet_amd import resample as R
    for p, q in ((1, 3), (441, 160), (160, 441)):
        half = 16 * max(p, q)
        tile = R.tile_outputs(p, q, half)
        big = -(-(2 * tile + 64) * q // p)                        # a packet of several tiles
        received = [0, 1000, 5, 77, 3 * big]
        emitted = [SR.ready(n, p, q, half) for n in received]
        lengths = [10, 0, big, 160, 1]                            # before the look-ahead, empty, several tiles, closing, one sample
        closing = [False, False, False, True, False]
        slots = [4, 0, 7, 2, 5]
        plan = R.plan_stream(received, emitted, lengths, closing, p, q, half, tile, slots)
        want = _loop_plan(received, emitted, lengths, closing, p, q, half, tile, slots)
        assert plan.table.dtype == np.int64 and plan.table.shape == (5, R.STREAM_INTS)
        assert plan.table.tolist() == want
        assert plan.lengths == [r[5] for r in want] and plan.out_off == [r[6] for r in want]
        assert plan.lengths[0] == 0 and plan.lengths[1] == 0 and plan.lengths[2] > 2 * tile
        assert plan.lengths[3] == -(-237 * p // q) - emitted[3]
        assert (plan.n_in, plan.n_out, plan.n_tiles) == (sum(lengths), sum(plan.lengths), want[-1][9])
        assert plan.received.tolist() == [10, 1000, 5 + big, 0, 3 * big + 1]
        assert plan.emitted.tolist() == [SR.ready(n, p, q, half) for n in (10, 1000, 5 + big)] + [0] + \
            [SR.ready(3 * big + 1, p, q, half)]
        assert plan.moves
        # nothing to move: empty packets and closing sessions only
        assert not R.plan_stream([5, 9], [0, 0], [0, 3], [False, True], p, q, half, tile).moves
    empty = R.plan_stream([], [], [], False, 1, 3, 48, 1280)
    assert empty.table.shape == (0, R.STREAM_INTS) and (empty.n_in, empty.n_out, empty.n_tiles) == (0, 0, 0)
    for kw in (dict(lengths=[1]), dict(lengths=[1, -1]), dict(lengths=[1.5, 2.0]), dict(received=[0, -1]),
               dict(emitted=[0, 400]), dict(slots=[3, 3]), dict(closing=[True]), dict(lengths=[2 ** 31, 1]),
               dict(lengths=[2 ** 30, 2 ** 30]), dict(received=[2 ** 41, 0], emitted=[0, 0], closing=True)):
        v = dict(dict(received=[0, 1000], emitted=[0, 318], lengths=[5, 5], closing=False, slots=None), **kw)
        with pytest.raises(ValueError):
            R.plan_stream(v["received"], v["emitted"], v["lengths"], v["closing"], 1, 3, 48, 1280, v["slots"])


def test_stream_resampler_refuses_misuse_before_any_device_work():
    from tinyrecurrentunet_amd import _lib
    from tinyrecurrentunet_amd import resample as R
    with pytest.raises(_lib.TrunetHipError):
        R.StreamResampler(48000, 16000, 4, device="cpu")
    for slots in (0, -1, 1.5):
        with pytest.raises(ValueError):
            R.StreamResampler(48000, 16000, slots)
    with pytest.raises(ValueError):
        R.StreamResampler(48000, 16001, 4)
    for fs_in in (48000, 16000):                                   # a real ratio and the identity
        sr = R.StreamResampler(fs_in, 16000, 4)
        sr._recv[:] = [0, 100, 200, 300]
        sr._emit[:] = [R.ready(n, sr.p, sr.q, sr.half) if not sr.identity else n for n in (0, 100, 200, 300)]
        before = (sr._recv.copy(), sr._emit.copy())
        ok = torch.zeros(160)
        with pytest.raises(_lib.TrunetHipError):
            sr.feed([ok, ok], [0, 1])                               # CPU tensors
        with pytest.raises(_lib.TrunetHipError):
            sr.feed((torch.zeros(320), [160, 160]), [0, 1])
        for packets, ids in (([ok], [4]), ([ok], [-1]), ([ok, ok], [1, 1]), ([ok], [0, 1]), ([ok, ok], [0]),
                             ([ok], [0.0]), ([torch.zeros(2, 80)], [0]), (ok, [0]),
                             ((torch.zeros(320), [160, 161]), [0, 1]), ((torch.zeros(320), [321, -1]), [0, 1])):
            with pytest.raises(ValueError):
                sr.feed(packets, ids)
        for ids in ([4], [0, 0], [[0, 1]]):
            with pytest.raises(ValueError):
                sr.close(ids)
            with pytest.raises(ValueError):
                sr.reset(ids)
        with pytest.raises(ValueError):
            sr.received(7)
        assert (sr._recv == before[0]).all() and (sr._emit == before[1]).all()
        assert sr._hist is None and sr._table is None              # nothing was allocated
        assert sr.feed([], []) == [] and sr.close([]) == []
        sr.reset([1, 3])
        assert [sr.received(i) for i in range(4)] == [0, 0, 200, 0] and sr.emitted(1) == 0 and sr.emitted(3) == 0


def _host_pool(fs, slots=4):
    """the host side of a StreamPool: everything its checks need, and no device"""
    from tinyrecurrentunet_amd import streaming as sm
    pool = sm.StreamPool.__new__(sm.StreamPool)
    pool._host_init(slots, fs, torch.device("cuda"))
    return pool


def test_stream_pool_at_another_rate_refuses_misuse_before_any_device_work():
    from tinyrecurrentunet_amd import _lib
    from tinyrecurrentunet_amd import resample as R
    for fs, short in ((48000, 768), (44100, 705)):                 # 256 samples at 16 kHz: one too few
        pool = _host_pool(fs)
        assert pool.fs == fs and pool.capacity == 4
        ids = pool.open(3)
        # a session that was fed `short` samples and one that was fed plenty; all of it is still inside the resampler
        # or the FIFO as far as the host counters go
        p, q, half = pool._down.p, pool._down.q, pool._down.half
        for i, n in zip(ids, (short, 48000, 0)):
            m = R.ready(n, p, q, half)
            pool._down._recv[i], pool._down._emit[i] = n, m
            pool._hops[i], pool._pend[i] = m // 128, m % 128
        state = lambda: (pool._hops.copy(), pool._pend.copy(), pool._down._recv.copy(), pool._down._emit.copy(),
                         pool._up._recv.copy(), pool._up._emit.copy(), pool._alloc.is_open.copy())
        before = state()
        with pytest.raises(ValueError, match="feed"):
            pool.step(torch.zeros(1, 128), [ids[1]])
        with pytest.raises(ValueError, match="feed"):
            pool.close([ids[1]], [torch.zeros(5)])
        with pytest.raises(ValueError, match="2 tails for 1 sessions"):
            pool.close([ids[1]], [None, None])                      # as the 16 kHz close refuses it
        with pytest.raises(_lib.TrunetHipError, match="the pool sits on"):
            pool.feed([torch.zeros(960)], [ids[1]])
        with pytest.raises(ValueError, match="at least 257"):
            pool.close([ids[1], ids[0]])                           # the short one; its call-mate stays open as well
        with pytest.raises(ValueError, match="at least 257"):
            pool.close([ids[2]])
        with pytest.raises(_lib.TrunetHipError):
            pool.feed([torch.zeros(960)], [ids[1]])                 # CPU tensors
        with pytest.raises(ValueError):
            pool.feed([torch.zeros(960)], [3])                      # not open
        with pytest.raises(ValueError):
            pool.feed([torch.zeros(960)] * 2, [ids[0], ids[0]])
        with pytest.raises(ValueError):
            pool.feed([torch.zeros(960)], [ids[0], ids[1]])
        for a, b in zip(before, state()):
            assert (a == b).all()
        assert pool._down._hist is None and pool._up._hist is None
        # abort and open reset both resamplers' counters of the slot
        pool.abort([ids[1]])
        assert pool._down.received(ids[1]) == 0 and pool._down.emitted(ids[1]) == 0
        pool._down._recv[ids[1]] = 99
        assert pool.open(1) == [ids[1]] and pool._down.received(ids[1]) == 0
    with pytest.raises(ValueError):
        _host_pool(44101)
    plain = _host_pool(16000)
    assert plain.fs == 16000 and plain._down is None and plain._up is None


def test_stream_entry_points_reject_null_and_bad_counts():
    """TRUNET_EINVAL on the host, no launch (the pattern of test_resample_cpu.test_entry_point_rejects_null_and_bad_shapes)"""
    from tinyrecurrentunet_amd import _lib
    lib, E = _lib.lib(), _lib.TRUNET_EINVAL
    # 48 kHz -> 16 kHz: p = 1, q = 3, half = 48, K = 97, tile 1280; 2 sessions, 3000 samples in, 1000 out, 2 tiles
    good = dict(hist=0x1000, inp=0x2000, out=0x3000, plan=0x4000, tab=0x5000, half=48, K=97, p=1, q=3, tile=1280, n_sess=2,
                slots=4, n_in=3000, n_out=1000, n_tiles=2, lds=1)

    def run(**kw):
        v = dict(good, **kw)
        return lib.trunet_resample_stream(v["hist"], v["inp"], v["out"], v["plan"], v["tab"], v["half"], v["K"], v["p"],
                                          v["q"], v["tile"], v["n_sess"], v["slots"], v["n_in"], v["n_out"], v["n_tiles"],
                                          v["lds"], None)

    def commit(**kw):
        v = dict(good, **kw)
        return lib.trunet_resample_stream_commit(v["hist"], v["inp"], v["plan"], v["half"], v["K"], v["p"], v["q"],
                                                 v["n_sess"], v["slots"], v["n_in"], None)

    ratio_cases = (dict(p=0), dict(q=0), dict(p=641, q=3, half=16 * 641, K=33), dict(q=641, half=16 * 641, K=2 * 16 * 641 + 1),
                   dict(half=47), dict(half=0, K=1), dict(half=33 * 3, K=199), dict(K=96), dict(K=98),
                   dict(p=1, q=640, half=32 * 640, K=2 * 32 * 640 + 1))       # a history beyond TRUNET_RS_STREAM_MAX_HISTORY
    for kw in (dict(hist=None), dict(inp=None), dict(out=None), dict(plan=None), dict(tab=None), dict(n_sess=0),
               dict(n_sess=-1), dict(slots=0), dict(n_in=-1), dict(n_out=-1), dict(n_tiles=-1), dict(n_in=2 ** 31),
               dict(n_out=2 ** 31, n_tiles=2 ** 31 // 1280 + 1), dict(n_tiles=0), dict(n_tiles=3), dict(tile=0),
               dict(tile=1000), dict(tile=8192), dict(lds=2), dict(lds=-1),
               dict(p=640, q=441, half=10240, K=33, tile=256, n_tiles=4, lds=1)) + ratio_cases:
        assert run(**kw) == E, kw
    assert run(n_out=0, n_tiles=0, out=None) == _lib.TRUNET_OK       # nothing to compute: no launch
    assert run(n_in=0, inp=None, n_out=0, n_tiles=0, out=None) == _lib.TRUNET_OK
    for kw in (dict(hist=None), dict(inp=None), dict(plan=None), dict(n_sess=0), dict(slots=0), dict(n_in=-1),
               dict(n_in=2 ** 31)) + ratio_cases:
        assert commit(**kw) == E, kw
    assert commit(n_in=0, inp=None) == _lib.TRUNET_OK                 # every packet empty: no launch
