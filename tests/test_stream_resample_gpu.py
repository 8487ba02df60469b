"""GPU: the stateful resampler (tinyrecurrentunet_amd/resample.py: StreamResampler, resample.hip)
and the stream pool at other rates than 16 kHz (streaming.py: StreamPool(fs=)).  The yardstick is bit-exactness: however a
session is cut into packets, what feed and close returned is torch.equal to the offline resampler on the whole."""
import numpy as np
import pytest
import torch

import resample_ref as RR

pytestmark = pytest.mark.gpu

# ratio -> (fs_in, fs_out); the last one is staged in several windows (the kernel's other path)
RATES = {(1, 3): (48000, 16000), (3, 1): (16000, 48000), (160, 441): (44100, 16000), (441, 160): (16000, 44100),
         (2, 1): (8000, 16000), (1, 6): (96000, 16000), (1, 40): (16000, 400)}
SENTINEL = 7.25


def _signal(n, seed, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _packets(x, cuts):
    edges = [0] + [int(c) for c in cuts] + [x.shape[0]]
    return [x[a:b] for a, b in zip(edges[:-1], edges[1:])]


def _drive(obj, sessions, on_feed=None):
    """sessions: {slot: list of packets}.  Step s feeds packet s of every session that still has one, in ONE call, then
    closes, in one call, the sessions whose last packet that was -- while the others go on.  -> {slot: feeds + close
    concatenated}.  obj: a StreamResampler or a StreamPool."""
    got = {s: [] for s in sessions}
    for step in range(max(len(p) for p in sessions.values())):
        live = [s for s, p in sessions.items() if step < len(p)]
        outs = obj.feed([sessions[s][step] for s in live], live)
        assert len(outs) == len(live)
        for s, o in zip(live, outs):
            got[s].append(o.clone())
        if on_feed is not None:
            on_feed(live, [sessions[s][step].shape[0] for s in live], outs)
        done = [s for s in live if step == len(sessions[s]) - 1]
        if done:
            for s, o in zip(done, obj.close(done)):
                got[s].append(o.clone())
    return {s: torch.cat(v) for s, v in got.items()}


def _random_cuts(n, seed, k=9):
    g = np.random.default_rng(seed)
    c = sorted(g.integers(0, n + 1, size=k).tolist())
    return c[:3] + [c[2]] + c[3:] + [c[-1]]                      # with empty packets


@pytest.mark.parametrize("pq", list(RATES))
def test_chunk_invariance_bit_for_bit(pq):
    from tinyrecurrentunet_amd import resample as R
    p, q = pq
    fs_in, fs_out = RATES[pq]
    sr = R.StreamResampler(fs_in, fs_out, 4)
    assert (sr.p, sr.q) == pq and sr.H == sr.K - 1 == R.history(p, sr.half)
    # a tile and 17 outputs' worth: samples after which a tile and 17 outputs are READY, so that one feed of them
    # owes more than a tile (the look-ahead holds the last ceil(half / q) outputs back until close)
    long_n = -(-((sr.tile + 17) * q + sr.half) // p)
    owed = R.ready(long_n, p, q, sr.half)
    assert sr.tile + 17 <= owed < sr.tile + 17 + 2 + p // q and R.ready(10, p, q, sr.half) == 0
    lens = [1, sr.K - 1, 1000, long_n]
    xs = [torch.from_numpy(_signal(n, 31 * p + q + i)).cuda() for i, n in enumerate(lens)]
    want = [R.resample([x], fs_in, fs_out)[0] for x in xs]
    for w, n in zip(want, lens):
        assert w.shape == (R.out_length(n, p, q),)
    every = lambda x, k: list(range(k, x.shape[0], k))
    styles = {
        "singles and 160s": [every(xs[0], 160), every(xs[1], 160), every(xs[2], 1), every(xs[3], 160)],
        "random cuts with empty packets": [_random_cuts(n, 5 * n + p) for n in lens],
        "a packet of more than a tile": [[], [], [999], [10]],
        "all at once": [[], [], [], []],
    }
    for name, cuts in styles.items():
        order = [2, 0, 3, 1] if name.startswith("random") else [0, 1, 2, 3]       # session i sits in slot order[i]
        most = {}                                                   # slot -> the most outputs one feed gave it

        def on_feed(live, ns, outs):
            for s, o in zip(live, outs):
                most[s] = max(most.get(s, 0), o.shape[0])

        got = _drive(sr, {order[i]: _packets(xs[i], cuts[i]) for i in range(4)}, on_feed)
        if name in ("a packet of more than a tile", "all at once"):
            assert most[order[3]] == owed > sr.tile, (pq, name, most)   # one launch, two tiles of one session
        for i in range(4):
            assert got[order[i]].shape == want[i].shape, (pq, name, i)
            assert torch.equal(got[order[i]], want[i]), (pq, name, i, float((got[order[i]] - want[i]).abs().max()))
            assert sr.received(order[i]) == 0 and sr.emitted(order[i]) == 0      # closed: the slot starts afresh


@pytest.mark.parametrize("pq", [(1, 3), (441, 160)])
def test_a_session_does_not_depend_on_its_mates_its_slot_or_the_order(pq):
    from tinyrecurrentunet_amd import resample as R
    p, q = pq
    fs_in, fs_out = RATES[pq]
    x = torch.from_numpy(_signal(5000, 77)).cuda()
    mates = [torch.from_numpy(_signal(n, 78 + n, scale=50.0)).cuda() for n in (4100, 7000, 2500)]
    pk = _packets(x, list(range(441, 5000, 441)))
    alone = _drive(R.StreamResampler(fs_in, fs_out, 1), {0: pk})[0]
    assert torch.equal(alone, R.resample([x], fs_in, fs_out)[0])
    sr = R.StreamResampler(fs_in, fs_out, 6)
    busy = _drive(sr, {0: _packets(mates[0], [700, 701, 3000]), 4: pk, 2: _packets(mates[1], list(range(160, 7000, 160))),
                       5: _packets(mates[2], [])})
    assert torch.equal(busy[4], alone)
    # another slot, the ids in another order, on the same resampler after the sessions above
    again = _drive(sr, {5: _packets(mates[1], [3000]), 3: _packets(mates[0], list(range(960, 4100, 960))), 1: pk})
    assert torch.equal(again[1], alone)
    assert torch.equal(again[5], busy[2]) and torch.equal(again[3], busy[0])


def test_state_hygiene():
    from tinyrecurrentunet_amd import _lib
    from tinyrecurrentunet_amd import resample as R
    fs_in, fs_out = 48000, 16000
    x = torch.from_numpy(_signal(3000, 5)).cuda()
    loud = torch.from_numpy(_signal(4000, 6, scale=1e4)).cuda()
    fresh = _drive(R.StreamResampler(fs_in, fs_out, 2), {1: _packets(x, [100, 960])})[1]
    sr = R.StreamResampler(fs_in, fs_out, 2)
    sr.feed([loud[:2500], loud[:1000]], [1, 0])
    sr.feed([loud[2500:]], [1])
    assert sr.received(1) == 4000 and sr.emitted(1) == R.ready(4000, sr.p, sr.q, sr.half)
    sr.reset([1])                                                   # the loud session is dropped in mid-stream
    assert sr.received(1) == 0 and sr.emitted(1) == 0 and sr.received(0) == 1000
    again = _drive(sr, {1: _packets(x, [100, 960])})[1]
    assert torch.equal(again, fresh) and torch.equal(fresh, R.resample([x], fs_in, fs_out)[0])
    # a raised misuse leaves every history and every counter as it was
    hist = sr.hist.clone()
    counts = (sr._recv.copy(), sr._emit.copy())
    ok = x[:160]
    for packets, ids, exc in (([ok.cpu()], [0], _lib.TrunetHipError), ([ok, ok], [0, 0], ValueError), ([ok], [2], ValueError),
                              ([ok, ok], [0], ValueError), ([ok.long()], [0], ValueError), ([ok.view(2, 80)], [0], ValueError),
                              ((x[:320], [160, 161]), [0, 1], ValueError)):
        with pytest.raises(exc):
            sr.feed(packets, ids)
    with pytest.raises(ValueError):
        sr.close([0, 2])
    assert torch.equal(sr.hist, hist) and (sr._recv == counts[0]).all() and (sr._emit == counts[1]).all()
    # the identity: copies, whatever the cut
    ident = R.StreamResampler(16000, 16000, 2)
    outs = ident.feed([x[:100], x[:0]], [1, 0])
    assert torch.equal(outs[0], x[:100]) and outs[0].data_ptr() != x.data_ptr() and outs[1].shape == (0,)
    assert ident.received(1) == ident.emitted(1) == 100 and ident.close([1])[0].shape == (0,) and ident.received(1) == 0


@pytest.mark.parametrize("pq", [(1, 3), (160, 441), (441, 160), (1, 40)])
def test_accuracy_against_float64(pq):
    """the derived bound of section 3l per output, (K + 3) 2^-24 p sum |h x|, on a stream fed in 160-sample packets"""
    from tinyrecurrentunet_amd import resample as R
    p, q = pq
    fs_in, fs_out = RATES[pq]
    x = _signal(6000, 9 * p + q)
    xt = torch.from_numpy(x).cuda()
    y = _drive(R.StreamResampler(fs_in, fs_out, 1), {0: _packets(xt, list(range(160, 6000, 160)))})[0].cpu().numpy()
    ref, a = RR.resample(x.astype(np.float64), p, q)
    assert y.shape == ref.shape
    bound = RR.bound(a, p, 16 * max(p, q))
    err = np.abs(y.astype(np.float64) - ref)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print("stream resample %d/%d: largest |err| / bound = %.4f" % (p, q, worst))
    assert np.all(err <= bound), (pq, worst)


def test_record_guards_and_refusals():
    """Records that leave the extents passed to the entry points are skipped by both kernels.  Every buffer -- the
    histories, the packed samples, the outputs -- is allocated with a margin on BOTH sides of the extents passed in (a
    history row, ``pad`` samples) and prefilled with a sentinel, and every bad record below points into those margins
    or, where its count is absurd, at samples the line defines as zero without reading memory: a missing guard fails the
    test, and cannot read or write outside an allocation."""
    from tinyrecurrentunet_amd import _lib
    from tinyrecurrentunet_amd import resample as R
    lib, st = _lib.lib(), _lib.stream()
    sr = R.StreamResampler(48000, 16000, 3)
    S, H, tile = 3, sr.H, sr.tile
    args = (sr.half, sr.K, sr.p, sr.q)
    table = sr.table
    pad = 2 * tile

    def margins(x):
        """x between ``pad`` sentinels on either side -> (the whole allocation, the view the entry points get)"""
        full = torch.full((x.shape[0] + 2 * pad,), SENTINEL, device="cuda")
        full[pad:pad + x.shape[0]] = x
        return full, full[pad:pad + x.shape[0]]

    def new_hist(rows=None):
        """(S + 2, H): a sentinel row before slot 0 and one after slot S - 1; rows: the S rows between"""
        full = torch.full((S + 2, H), SENTINEL, device="cuda")
        if rows is not None:
            full[1:S + 1] = rows
        return full

    lens = [500, 2 * tile * 3 + 100, 300]                          # the middle session: more than two tiles of outputs
    _, x0 = margins(torch.from_numpy(_signal(3 * 400, 1)).cuda())
    _, x1 = margins(torch.from_numpy(_signal(sum(lens), 2)).cuda())
    plan0 = R.plan_stream([0] * 3, [0] * 3, [400] * 3, False, *args[2:], sr.half, tile, [0, 1, 2])
    plan1 = R.plan_stream(plan0.received, plan0.emitted, lens, [False, False, True], *args[2:], sr.half, tile, [0, 1, 2])

    def call(plan, tab, samples, hist_full):
        """-> (the whole output allocation, its n_out outputs); hist_full: (S + 2, H), the entry points get rows 1 .. S"""
        out_full, out = margins(torch.full((plan.n_out,), SENTINEL, device="cuda"))
        hist = hist_full[1:]
        dev_tab = torch.from_numpy(tab).cuda()
        rc = lib.trunet_resample_stream(hist.data_ptr(), samples.data_ptr(), out.data_ptr(), dev_tab.data_ptr(),
                                        table.data_ptr(), *args, tile, len(tab), S, plan.n_in, plan.n_out, plan.n_tiles, 1, st)
        assert rc == 0
        rc = lib.trunet_resample_stream_commit(hist.data_ptr(), samples.data_ptr(), dev_tab.data_ptr(), *args, len(tab), S,
                                               plan.n_in, st)
        assert rc == 0
        return out_full, out

    def margins_intact(out_full, n_out, hist_full):
        return bool((out_full[:pad] == SENTINEL).all() and (out_full[pad + n_out:] == SENTINEL).all()
                    and (hist_full[0] == SENTINEL).all() and (hist_full[S + 1] == SENTINEL).all())

    hist0 = new_hist()
    full0, out0 = call(plan0, plan0.table, x0, hist0)
    assert margins_intact(full0, plan0.n_out, hist0)
    hist_good = hist0.clone()
    fullg, good = call(plan1, plan1.table, x1, hist_good)
    seg = [slice(o, o + m) for o, m in zip(plan1.out_off, plan1.lengths)]
    assert plan1.lengths[1] > 2 * tile and margins_intact(fullg, plan1.n_out, hist_good)
    # the good run is the stream resampler's own
    a = sr.feed(list(torch.split(x0, 400)), [0, 1, 2])
    b = sr.feed(list(torch.split(x1, lens))[:2], [0, 1]) + sr.feed([x1[sum(lens[:2]):]], [2], closing=True)
    for i in range(3):
        assert torch.equal(out0[plan0.out_off[i]:plan0.out_off[i] + plan0.lengths[i]], a[i]) and torch.equal(good[seg[i]], b[i])
    assert torch.equal(hist_good[1:3], sr.hist[:2])
    assert torch.equal(hist_good[3], hist0[3])                      # a closing session keeps no history

    # (column, value) of the middle record.  Without its guard a record would touch: slot S / -1: the history row after /
    # before the extent; an output or packet extent one past / one before: the first / last sample of a margin; an output
    # or packet count beyond the extent: less than a tile of outputs, or the packet's offset in samples, past it (pad is
    # wider); a count of -1, or one
    # beyond 2^40 / 2^50: samples outside [0, N1) or below the history, which the line gives as zero without a read.
    assert max(plan1.out_off[1], lens[0], tile) + 1 <= pad
    cases = [(0, S), (0, -1),                                       # the slot
             (6, plan1.n_out - plan1.lengths[1] + 1), (6, -1), (5, plan1.n_out + 1),                 # the output extent
             (3, plan1.n_in), (2, plan1.n_in - lens[1] + 1), (2, -1), (3, -1),                       # the packet extent
             (1, -1), (1, 2 ** 41), (4, -1), (4, 2 ** 51),                                           # the counters
             (9, plan1.n_tiles + 1)]                                # the tiles
    for col, value in cases:
        tab = plan1.table.copy()
        tab[1, col] = value
        hist = hist0.clone()
        full, out = call(plan1, tab, x1, hist)
        assert (out[seg[1]] == SENTINEL).all(), (col, value)       # skipped: nothing of it was written
        assert margins_intact(full, plan1.n_out, hist), (col, value)
        assert torch.equal(out[seg[0]], good[seg[0]]) and torch.equal(hist[1], hist_good[1]), (col, value)
        if col in (0, 1, 2, 3):                                     # what the commit kernel checks too: its history stays
            assert torch.equal(hist[2], hist0[2]), (col, value)
        if col != 9:                                                # the last session's tiles follow the changed record
            assert torch.equal(out[seg[2]], good[seg[2]]), (col, value)
    hist0 = hist0[1:S + 1].clone()                                  # from here on: the S rows alone
    # TRUNET_EINVAL without a launch
    E = _lib.TRUNET_EINVAL
    out = torch.full((plan1.n_out,), SENTINEL, device="cuda")
    tab = torch.from_numpy(plan1.table).cuda()
    hist = hist0.clone()
    ptrs = dict(hist=hist.data_ptr(), inp=x1.data_ptr(), out=out.data_ptr(), plan=tab.data_ptr(), tab=table.data_ptr())
    nums = dict(half=sr.half, K=sr.K, p=sr.p, q=sr.q, tile=tile, n_sess=3, slots=S, n_in=plan1.n_in, n_out=plan1.n_out,
                n_tiles=plan1.n_tiles, lds=1)

    def run(**kw):
        v = dict(ptrs, **nums)
        v.update(kw)
        return lib.trunet_resample_stream(v["hist"], v["inp"], v["out"], v["plan"], v["tab"], v["half"], v["K"], v["p"],
                                          v["q"], v["tile"], v["n_sess"], v["slots"], v["n_in"], v["n_out"], v["n_tiles"],
                                          v["lds"], st)

    def commit(**kw):
        v = dict(ptrs, **nums)
        v.update(kw)
        return lib.trunet_resample_stream_commit(v["hist"], v["inp"], v["plan"], v["half"], v["K"], v["p"], v["q"],
                                                 v["n_sess"], v["slots"], v["n_in"], st)

    for kw in (dict(hist=None), dict(inp=None), dict(out=None), dict(plan=None), dict(tab=None), dict(n_sess=0), dict(slots=0),
               dict(p=0), dict(q=641), dict(half=47), dict(K=96), dict(tile=1000), dict(n_in=-1), dict(n_out=-1),
               dict(n_tiles=plan1.n_tiles + 3), dict(n_tiles=0), dict(lds=2)):
        assert run(**kw) == E, kw
    for kw in (dict(hist=None), dict(inp=None), dict(plan=None), dict(n_sess=0), dict(slots=0), dict(K=98), dict(n_in=-1)):
        assert commit(**kw) == E, kw
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and torch.equal(hist, hist0)     # nothing was launched


# ---------------------------------------------------------------- the pool at another rate
_NETS = {}


def _net(cin, use_tgru=False):
    from oracle import network_ref as nr, weights as W
    from tinyrecurrentunet_amd import network as hn
    key = (cin, use_tgru)
    if key not in _NETS:
        net = hn.TRUNet(input_size=cin, use_tgru=use_tgru)
        net.load_state_dict(W.fill_state_dict(nr.TRUNet(input_size=cin), seed=5).state_dict())
        _NETS[key] = net.cuda().eval()
    return _NETS[key]


def _rel_l2(y, r):
    y, r = y.double(), r.double()
    return float((y - r).norm() / (r.norm() + 1e-300))


def _pool_sessions(fs, seed):
    """three sessions of different lengths, each cut its own way: 20 ms packets, random cuts with empty packets, 441s; the
    shortest closes while the others go on"""
    lens = [fs // 4 + 7, fs // 3 + 1, 2 * fs // 5 + 250]
    xs = [torch.from_numpy(_signal(n, seed + i, scale=0.1)).cuda() for i, n in enumerate(lens)]
    cuts = [list(range(fs // 50, lens[0], fs // 50)), _random_cuts(lens[1], seed, k=12), list(range(441, lens[2], 441))]
    return xs, cuts


_POOL_RUNS = {}


def _pool_run(cin, tgru, fs):
    """the three sessions through a pool at fs -> (xs, results); every call's lengths are checked against the host
    formula on the way"""
    from tinyrecurrentunet_amd import resample as R
    key = (cin, tgru, fs)
    if key in _POOL_RUNS:
        return _POOL_RUNS[key]
    net = _net(cin, tgru)
    xs, cuts = _pool_sessions(fs, 40 + cin)
    pool = net.stream_pool(4, fs=fs)
    assert pool.fs == fs and pool.tgru == tgru
    ids = pool.open(3)
    pd, qd = R.ratio(fs, 16000)
    pu, qu = R.ratio(16000, fs)
    hd, hu = 16 * max(pd, qd), 16 * max(pu, qu)
    fed = {s: 0 for s in ids}
    sent = {s: 0 for s in ids}

    def on_feed(live, ns, outs):
        """ready_up of the 16 kHz samples delivered so far, minus what was already emitted"""
        for s, n, o in zip(live, ns, outs):
            fed[s] += n
            n16 = R.ready(fed[s], pd, qd, hd)                       # samples that have reached the 16 kHz pool
            assert pool.hops(s) == n16 // 128 and pool.pending(s) == n16 % 128
            delivered = 128 * max(n16 // 128 - 3, 0)                # ... and left it
            assert o.shape[0] == R.ready(delivered, pu, qu, hu) - sent[s], (s, fed[s], o.shape)
            sent[s] += o.shape[0]

    got = _drive(pool, {ids[i]: _packets(xs[i], cuts[i]) for i in range(3)}, on_feed)
    assert pool.free == 4
    res = [got[ids[i]] for i in range(3)]
    for x, y in zip(xs, res):
        assert y.shape == x.shape and torch.isfinite(y).all()       # after close: exactly the samples it was fed
    _POOL_RUNS[key] = (xs, res)
    return xs, res


@pytest.mark.parametrize("fs", [48000, 44100])
@pytest.mark.parametrize("tgru", [False, True])
@pytest.mark.parametrize("cin", [3, 4])
def test_pool_at_another_rate_is_the_exact_composition(cin, tgru, fs):
    from tinyrecurrentunet_amd import resample as R
    net = _net(cin, tgru)
    xs, res = _pool_run(cin, tgru, fs)
    plain = net.stream_pool(2)
    for x, y in zip(xs, res):
        x16 = R.resample([x], fs, 16000)[0]
        s, = plain.open(1)
        ys16 = torch.cat([plain.feed([x16], [s])[0], plain.close([s])[0]])
        assert ys16.shape == x16.shape
        want = R.resample([ys16], 16000, fs)[0][:x.shape[0]]
        assert torch.equal(y, want), float((y - want).abs().max())


@pytest.mark.parametrize("kind", ["fp32", "tgru", "int8"])
def test_pool_at_another_rate_against_offline_enhancement(kind):
    """twice the bound of test_stream_pool_gpu for the same kind: the up-resampler is a linear filter of gain at most
    +0.01 dB, so it cannot enlarge the difference, and it may shrink the reference's norm by what it cuts above 0.94 of
    8 kHz"""
    from tinyrecurrentunet_amd.enhance import enhance
    fs = 48000
    if kind == "int8":
        net = _net(4)
        xs, cuts = _pool_sessions(fs, 44)
        pool = net.stream_pool(4, fs=fs, int8=True)
        ids = pool.open(3)
        got = _drive(pool, {ids[i]: _packets(xs[i], cuts[i]) for i in range(3)})
        res = [got[i] for i in ids]
    else:
        net = _net(4, kind == "tgru")
        xs, res = _pool_run(4, kind == "tgru", fs)
    for x, y in zip(xs, res):
        ref = enhance(net, [x], fs=fs, path="int8" if kind == "int8" else "auto")[0]
        assert ref.shape == y.shape == x.shape
        rel, worst = _rel_l2(y, ref), float((y - ref).abs().max() / ref.abs().max())
        print("pool at %d Hz, %s, %d samples: relative L2 %.3e, max |diff| / max |ref| %.3e" % (fs, kind, x.shape[0], rel, worst))
        if kind == "int8":
            assert worst <= 2 * 1e-2, worst
        else:
            assert rel < 2 * (1e-4 if kind == "tgru" else 1e-5), rel


def test_a_pool_at_16_khz_is_the_pool_without_fs():
    net = _net(4)
    x = torch.from_numpy(_signal(3000, 8, scale=0.1)).cuda()
    pk = _packets(x, [160, 161, 900, 2500])
    a, b = net.stream_pool(2, fs=16000), net.stream_pool(2)
    assert a.fs == b.fs == 16000
    ia, ib = a.open(1), b.open(1)
    ya, yb = _drive(a, {ia[0]: pk})[ia[0]], _drive(b, {ib[0]: pk})[ib[0]]
    assert ya.shape == x.shape and torch.equal(ya, yb)
    # step() and close(tails) stay with the 16 kHz pool, and are refused at another rate
    c = net.stream_pool(2, fs=48000)
    ic = c.open(1)
    with pytest.raises(ValueError, match="feed"):
        c.step(x[:128].view(1, 128), ic)
    with pytest.raises(ValueError, match="feed"):
        c.close(ic, [x[:5]])
    c.feed([x[:700]], ic)
    with pytest.raises(ValueError, match="at least 257"):
        c.close(ic)                                                 # 234 samples at 16 kHz: it stays open
    assert c.free == 1 and c._down.received(ic[0]) == 700
    c.abort(ic)
    assert c.free == 2 and c._down.received(ic[0]) == 0
