"""GPU: the band above 8 kHz in the stream pool above 16 kHz (tinyrecurrentunet_amd/stream_highband.py,
stream_highband.hip, StreamPool(highband=)).  "keep" is held to bit-exactness against the offline
``highband.rejoin`` however a session is cut; the causal "follow" to the float64 restatement
(tests/stream_highband_ref.py) within derived rounding bounds; both to bit-for-bit independence of cuts, pool-mates, slot
ids and runs.

Largest |err| / bound observed on the MI355X:
    block gains     0.0033  (a worst-case bound over 63 taps and 512 squares)
    join "follow"   0.41    (48 kHz 0.410, 44.1 kHz 0.327)"""
import numpy as np
import pytest
import torch

import highband_ref as HR
import stream_highband_ref as SR

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
SENTINEL = 7.25
RATES = (48000, 44100)
_NETS, _REFS, _RUNS = {}, {}, {}


def _signal(n, seed, scale=0.1):
    return (scale * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _slow(n, seed):
    """a slowly varying factor in [0, 1.5]"""
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.75 + 0.75 * np.sin(2 * np.pi * g.uniform(2.0, 9.0) * t + g.uniform(0, 6.0))).astype(np.float32)


def _net(cin, use_tgru=False):
    from oracle import network_ref as nr, weights as W
    from tinyrecurrentunet_amd import network as hn
    key = (cin, use_tgru)
    if key not in _NETS:
        net = hn.TRUNet(input_size=cin, use_tgru=use_tgru)
        net.load_state_dict(W.fill_state_dict(nr.TRUNet(input_size=cin), seed=5).state_dict())
        _NETS[key] = net.cuda().eval()
    return _NETS[key]


KINDS = {"c4": (4, False, False), "c3": (3, False, False), "tgru": (4, True, False), "int8": (4, False, True)}


def _pool(kind, slots, **kw):
    cin, tgru, int8 = KINDS[kind]
    return _net(cin, tgru).stream_pool(slots, int8=int8, **kw)


def _lengths(fs):
    from tinyrecurrentunet_amd import resample as R
    pd, qd = R.ratio(fs, 16000)
    first = 256 * qd // pd + 1                                      # the shortest with ceil(L pd / qd) = 257
    assert R.out_length(first, pd, qd) == 257 and R.out_length(first - 1, pd, qd) == 256
    return {"A": [first, first + 1, 8195], "B": [12007, 16001, 19450]}


def _sessions(fs, group):
    return [torch.from_numpy(_signal(n, 7 * n + fs % 97)).cuda() for n in _lengths(fs)[group]]


def _cut(n, how, seed=0):
    """packet boundaries of a session of n samples"""
    if how == "all":
        return []
    if how == "random":
        g = np.random.default_rng(seed + n)
        c = sorted(g.integers(0, n + 1, size=9).tolist())
        return c[:3] + [c[2]] + c[3:] + [c[-1]]                    # with empty packets
    return list(range(how, n, how))


def _packets(x, cuts):
    edges = [0] + [int(c) for c in cuts] + [x.shape[0]]
    return [x[a:b] for a, b in zip(edges[:-1], edges[1:])]


def _drive(pool, sessions, counts=None):
    """sessions: {slot: list of packets}.  Step s feeds packet s of every session that still has one, in ONE call, then
    closes, in one call, the sessions whose last packet that was -- while the others go on -> {slot: feeds + close
    concatenated}; counts: a list that receives the samples every feed returned"""
    got = {s: [] for s in sessions}
    for step in range(max(len(p) for p in sessions.values())):
        live = [s for s, p in sessions.items() if step < len(p)]
        outs = pool.feed([sessions[s][step] for s in live], live)
        if counts is not None:
            counts.append([int(o.shape[0]) for o in outs])
        for s, o in zip(live, outs):
            got[s].append(o.clone())
        done = [s for s in live if step == len(sessions[s]) - 1]
        if done:
            for s, o in zip(done, pool.close(done)):
                got[s].append(o.clone())
    return {s: torch.cat(v) for s, v in got.items()}


def _reference(kind, fs, group):
    """per session of the group: (x, lo, ys16) with lo the offline down-resampling and ys16 the plain 16 kHz pool's result"""
    from tinyrecurrentunet_amd import resample as R
    key = (kind, fs, group)
    if key not in _REFS:
        plain = _pool(kind, 2)
        res = []
        for x in _sessions(fs, group):
            lo = R.resample([x], fs, 16000)[0]
            s, = plain.open(1)
            ys16 = torch.cat([plain.feed([lo], [s])[0], plain.close([s])[0]])
            assert ys16.shape == lo.shape
            res.append((x, lo, ys16))
        _REFS[key] = res
    return _REFS[key]


def _run(kind, fs, group, mode, hows, slots=4, skip=0, counts=None, **kw):
    """the group's three sessions at once through a pool at fs, each cut its own way; skip: slots opened first and left idle"""
    key = (kind, fs, group, mode, tuple(hows), slots, skip, tuple(sorted(kw.items())))
    if key in _RUNS and counts is None:
        return _RUNS[key]
    xs = _sessions(fs, group)
    pool = _pool(kind, slots, fs=fs, highband=mode, **kw) if mode is not None else _pool(kind, slots, fs=fs)
    ids = pool.open(skip + 3)[skip:]
    got = _drive(pool, {s: _packets(x, _cut(x.shape[0], how, s)) for s, x, how in zip(ids, xs, hows)}, counts)
    assert pool.free == slots - skip
    res = [got[s] for s in ids]
    for x, y in zip(xs, res):
        assert y.shape == x.shape and torch.isfinite(y).all()
    _RUNS[key] = res
    return res


# ---------------------------------------------------------------- 1. "keep" is the offline rejoin, bit for bit
KEEP_CASES = [("c4", "A", (160, 960, "random")), ("c4", "A", ("all", "random", 160)), ("c4", "B", (960, "all", "random")),
              ("c3", "A", (160, "random", "all")), ("c3", "B", ("random", 960, 160)), ("tgru", "A", (960, "random", "all")),
              ("int8", "A", ("random", 160, 960))]


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("kind,group,hows", KEEP_CASES)
def test_keep_is_the_offline_rejoin_bit_for_bit(kind, group, hows, fs):
    from tinyrecurrentunet_amd import highband as HB
    res = _run(kind, fs, group, "keep", hows)
    for (x, lo, ys16), y in zip(_reference(kind, fs, group), res):
        want = HB.rejoin([x], [lo], [ys16], fs, "keep")[0]
        assert torch.equal(y, want), (x.shape[0], float((y - want).abs().max()))


# ---------------------------------------------------------------- 2. "follow" against the float64 restatement
def test_block_gains_match_the_restatement():
    """Gaussian lo, ys16 = lo m with a slowly varying m in [0, 1.5], and the lo / ys16 of a real session; the bound is
    stream_highband_ref.block_gains' own"""
    from tinyrecurrentunet_amd import highband as HB, stream_highband as SH
    lens = [257, 383, 384, 385, 511, 512, 513, 4803]
    lo = [_signal(n, 11 * n, 1.0) for n in lens]
    ys = [x * _slow(n, n) for x, n in zip(lo, lens)]
    for _, l, y in _reference("c4", 48000, "A")[2:]:
        lo.append(l.cpu().numpy())
        ys.append(y.cpu().numpy())
    gs = SH.block_gains([torch.from_numpy(v).cuda() for v in lo], [torch.from_numpy(v).cuda() for v in ys])
    torch.cuda.synchronize()
    g_min = HB.floor_gain(-30.0)
    worst = 0.0
    for x, y, g in zip(lo, ys, gs):
        n = x.shape[0]
        assert g.dtype == torch.float32 and g.shape == (-(-n // 128),)
        ref, bound = SR.block_gains(x.astype(np.float64), y.astype(np.float64), g_min=g_min)
        err = np.abs(g.cpu().numpy().astype(np.float64) - ref)
        ratio = float(np.max(err / bound))
        print("block gains L16 = %d: largest |err| / bound = %.4f (bound at most %.2e)" % (n, ratio, bound.max()))
        assert np.all(err <= bound), (n, ratio, int(np.argmax(err / bound)))
        assert g_min <= float(g.min()) and float(g.max()) <= 1.0
        worst = max(worst, ratio)
    print("block gains: largest |err| / bound = %.4f" % worst)


def test_block_gains_exact_cases():
    from tinyrecurrentunet_amd import highband as HB, stream_highband as SH
    lens = [257, 2049, 4803]
    lo = [torch.from_numpy(_signal(n, 3 * n, 1.0)).cuda() for n in lens]
    zeros = [torch.zeros_like(x) for x in lo]
    quarter = SH.block_gains(lo, [0.25 * x for x in lo])
    silent = SH.block_gains(zeros, zeros)
    removed = SH.block_gains(lo, zeros)
    deeper = SH.block_gains(lo, zeros, floor_db=-60.0)
    louder = SH.block_gains(lo, [3.0 * x for x in lo])
    for q, s, r, d, a in zip(quarter, silent, removed, deeper, louder):
        assert float((q - 0.25).abs().max()) <= 2 * 2.0 ** -25                # 2 ulp of 0.25, before and once four blocks exist
        assert torch.equal(s, torch.ones_like(s)) and torch.equal(a, torch.ones_like(a))
        assert torch.equal(r, torch.full_like(r, HB.floor_gain(-30.0)))
        assert torch.equal(d, torch.full_like(d, HB.floor_gain(-60.0)))


def _join_bound(up_y, up_x, x, G):
    """three roundings of the sum and three of the interpolation, with or without fused multiply-add (section 3p)"""
    return 4 * U32 * np.abs(up_y) + 8 * U32 * G * (np.abs(x) + np.abs(up_x))


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("group,hows", [("A", (160, 960, "random")), ("B", ("random", "all", 960))])
def test_follow_join_matches_float64(group, hows, fs):
    """the streamed "follow" against up_y + G (x - up_x) in float64 from the fp32 up_y and up_x of the offline resampler (the
    stream's are bit for bit those), the same x and the kernel's own block gains"""
    from tinyrecurrentunet_amd import resample as R, stream_highband as SH
    pd, qd = R.ratio(fs, 16000)
    res = _run("c4", fs, group, "follow", hows)
    worst = 0.0
    for (x, lo, ys16), y in zip(_reference("c4", fs, group), res):
        n = x.shape[0]
        up_y, up_x = R.resampler(16000, fs, "cuda")([ys16], x2=[lo])
        g = SH.block_gains([lo], [ys16])[0]
        x64, uy, ux = (v.cpu().numpy().astype(np.float64)[:n] for v in (x, up_y[0], up_x[0]))
        G = SR.sample_gains(g.cpu().numpy().astype(np.float64), n, pd, qd)
        ref = HR.join(uy, ux, x64, G)
        bound = _join_bound(uy, ux, x64, G)
        err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
        ratio = float(np.max(err / np.maximum(bound, 1e-300)))
        assert np.all(err <= bound), (fs, n, ratio, int(np.argmax(err / np.maximum(bound, 1e-300))))
        worst = max(worst, ratio)
    print("follow join at %d Hz, group %s: largest |err| / bound = %.4f" % (fs, group, worst))


# ---------------------------------------------------------------- 3. cuts, pool-mates, slots and runs change no bit
@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("mode", ["keep", "follow"])
def test_a_session_depends_on_nothing_but_its_samples(mode, fs):
    kw = dict(highband_floor_db=-40.0) if mode == "follow" else {}
    a = _run("c4", fs, "A", mode, (160, 960, "random"), **kw)
    b = _run("c4", fs, "A", mode, ("all", "random", 441), slots=7, skip=3, **kw)          # other cuts, other slot ids
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    xs = _sessions(fs, "A")
    pool = _pool("c4", 3, fs=fs, highband=mode, **kw)
    for i, how in ((2, 1000), (0, "all"), (2, "random")):                                # alone, and on a second run
        s = pool.open(2)[1]
        y = _drive(pool, {s: _packets(xs[i], _cut(xs[i].shape[0], how, 5))})[s]
        assert torch.equal(y, a[i]), (i, how)
        pool.abort([t for t in range(3) if pool._alloc.is_open[t]])


# ---------------------------------------------------------------- 4. a tone above the network's band
def _amplitude(v, f0, fs):
    """amplitude of the component at f0 over the middle half of v"""
    n = np.arange(v.shape[0])
    m = slice(v.shape[0] // 4, 3 * v.shape[0] // 4)
    return 2.0 * np.abs(np.sum(v[m].astype(np.float64) * np.exp(-2j * np.pi * f0 * n[m] / fs))) / (m.stop - m.start)


def test_a_12_khz_tone_is_lost_by_drop_and_returned_by_keep():
    fs, n = 48000, 14400
    sig = _signal(n, 21)
    spec = np.fft.rfft(sig)
    spec[int(3000.0 * n / fs):] = 0.0                                             # noise below 3 kHz + the tone
    x = (np.fft.irfft(spec, n) + 0.1 * np.sin(2 * np.pi * 12000.0 * np.arange(n) / fs + 0.3)).astype(np.float32)
    x = torch.from_numpy(x).cuda()
    amp = {}
    for mode in ("drop", "keep", "follow"):
        pool = _pool("c4", 2, fs=fs, highband=mode)
        assert pool.highband == mode and pool.highband_floor_db == -30.0
        s, = pool.open(1)
        y = _drive(pool, {s: _packets(x, _cut(n, 960))})[s]
        amp[mode] = _amplitude(y.cpu().numpy(), 12000.0, fs)
    print("12 kHz at 48 kHz through the pool: drop %.3e, keep %.6f, follow %.6f" % (amp["drop"], amp["keep"], amp["follow"]))
    assert amp["drop"] < 1e-6
    assert abs(amp["keep"] - 0.1) <= 0.01 * 0.1                                   # section 3p's tolerance for the offline path
    assert 10 ** -1.5 * 0.1 * 0.99 <= amp["follow"] <= 0.1 * 1.01


# ---------------------------------------------------------------- 5., 6. "drop", and the sample counts of feed
@pytest.mark.parametrize("fs", RATES)
def test_drop_is_the_pool_without_the_argument_and_feed_returns_its_counts(fs):
    hows = (160, 960, "random")
    n_plain, n_drop, n_keep, n_follow = [], [], [], []
    plain = _run("c4", fs, "A", None, hows, counts=n_plain)
    drop = _run("c4", fs, "A", "drop", hows, counts=n_drop)
    _run("c4", fs, "A", "keep", hows, counts=n_keep)
    _run("c4", fs, "A", "follow", hows, counts=n_follow)
    for u, v in zip(plain, drop):
        assert torch.equal(u, v)
    assert n_plain == n_drop == n_keep == n_follow and sum(map(sum, n_plain)) > 0      # call by call, no added latency
    pool = _pool("c4", 2, fs=fs, highband="drop")
    assert pool._hb is None


@pytest.mark.parametrize("fs", [16000, 8000])
def test_at_or_below_16_khz_follow_is_drop(fs):
    x = torch.from_numpy(_signal(3000 if fs == 16000 else 1500, 8)).cuda()
    res = []
    for kw in (dict(), dict(highband="follow", highband_floor_db=-20.0), dict(highband="keep")):
        pool = _pool("c4", 2, fs=fs, **kw)
        assert pool._hb is None                                                  # nothing new is allocated
        s, = pool.open(1)
        res.append(_drive(pool, {s: _packets(x, [160, 161, 900])})[s])
    assert torch.equal(res[0], res[1]) and torch.equal(res[0], res[2]) and res[0].shape == x.shape
    pool = _pool("c4", 2, fs=48000, highband="keep")
    ids = pool.open(1)
    with pytest.raises(ValueError, match="feed"):
        pool.step(x[:128].view(1, 128), ids)                                     # step stays a 16 kHz call
    with pytest.raises(ValueError):
        pool.close(ids, [x[:5]])


# ---------------------------------------------------------------- 7. refusals and guards
@pytest.mark.parametrize("mode", ["keep", "follow"])
def test_a_refused_call_changes_nothing(mode):
    fs = 48000
    xs = _sessions(fs, "A")
    want = _run("c4", fs, "A", mode, (480, 480, 480))
    pool = _pool("c4", 4, fs=fs, highband=mode)
    ids = pool.open(3)
    pk = [_packets(x, _cut(x.shape[0], 480)) for x in xs]
    got = [[], [], []]
    for step in range(len(pk[2])):
        live = [i for i in range(3) if step < len(pk[i])]
        if step in (1, 5):
            with pytest.raises(ValueError):
                pool.feed([pk[i][step] for i in live] + [pk[0][0]], [ids[i] for i in live] + [3])     # slot 3 is not open
        if step == 1:
            with pytest.raises(ValueError):
                pool.feed([pk[i][step] for i in live], [ids[live[0]]] * len(live))                    # a slot listed twice
            with pytest.raises(ValueError, match="257"):
                pool.close([ids[2], ids[0]])                                     # 480 samples fed: 160 at 16 kHz
        for i, o in zip(live, pool.feed([pk[i][step] for i in live], [ids[i] for i in live])):
            got[i].append(o.clone())
        done = [i for i in live if step == len(pk[i]) - 1]
        if done:
            for i, o in zip(done, pool.close([ids[i] for i in done])):
                got[i].append(o.clone())
    for g, w in zip(got, want):
        assert torch.equal(torch.cat(g), w)


def test_records_that_leave_the_extents_are_skipped():
    """Every buffer the entry points get lies between sentinel margins (a row of per-slot state, ``pad`` samples), and every
    bad record below points into those margins or is inconsistent in itself: a missing guard fails the test and cannot
    touch memory outside an allocation."""
    from tinyrecurrentunet_amd import _lib, highband as HB, stream_highband as SH
    lib, st = _lib.lib(), _lib.stream()
    S, xcap, pad = 3, SH.x_line_bound(1, 3), 4096
    g = torch.Generator(device="cuda").manual_seed(3)
    rnd = lambda *s: torch.randn(s, device="cuda", generator=g) * 0.1

    def margins(x):
        full = torch.full((x.shape[0] + 2 * pad,), SENTINEL, device="cuda")
        full[pad:pad + x.shape[0]] = x
        return full, full[pad:pad + x.shape[0]]

    def rows(*shape):
        """(S + 2, ...): a sentinel row before slot 0 and one after slot S - 1"""
        full = torch.full((S + 2,) + shape, SENTINEL, device="cuda")
        full[1:S + 1] = rnd(S, *shape)
        return full

    plan = SH.plan_highband(slots=[0, 1, 2], x_count=[500, 700, 300], lo_count=[200, 400, 100], blocks=[3, 5, 2],
                            emitted=[1000, 1900, 700], packet_lens=[960, 2500, 960], x16_lens=[320, 833, 320],
                            pair_lens=[256, 1152, 256], up_off=[0, 700, 3300], out_lens=[700, 2600, 600], n_up=3900,
                            closing=False, xcap=xcap)
    n = 3
    assert plan.n_join_tiles == 5 and plan.n_pair_tiles == 4 and plan.n_blocks == 13
    ext = (n, S, xcap, plan.n_packet, plan.n_up, plan.n_x16, plan.n_paired, plan.n_blocks)
    state0 = dict(x_line=rows(xcap), lo_line=rows(SH.LO_LINE), halo=rows(SH.HALO, 2), energy=rows(3, 2).abs(), gain=rows(2).abs())
    packet, x16, ys16 = (margins(rnd(k))[1] for k in (plan.n_packet, plan.n_x16, plan.n_paired))
    up_y, up_x = margins(rnd(plan.n_up))[1], margins(rnd(plan.n_up))[1]
    hp = HB._taps(torch.device("cuda"))

    def call(table):
        """all four entry points on a fresh copy of the state -> (state, outputs), each output inside its margins"""
        s = {k: v.clone() for k, v in state0.items()}
        v = {k: t[1:] for k, t in s.items()}                          # the entry points get rows 1 .. S
        tab = torch.from_numpy(table).cuda()
        o = dict(paired=margins(torch.full((plan.n_paired,), SENTINEL, device="cuda")),
                 eline=margins(torch.full((2 * (plan.n_blocks + 3 * n),), SENTINEL, device="cuda")),
                 gline=margins(torch.full((plan.n_blocks + 2 * n,), SENTINEL, device="cuda")),
                 out=margins(torch.full((plan.n_up,), SENTINEL, device="cuda")))
        P = lambda t: t.data_ptr()
        assert lib.trunet_stream_highband_pair(P(v["lo_line"]), P(x16), P(o["paired"][1]), P(tab), *ext, plan.n_pair_tiles,
                                               st) == 0
        assert lib.trunet_stream_highband_gains(P(o["paired"][1]), P(ys16), P(v["halo"]), P(v["energy"]), P(v["gain"]), P(hp),
                                                P(o["eline"][1]), P(o["gline"][1]), P(tab), *ext, 0.03, st) == 0
        assert lib.trunet_stream_highband_join(P(up_y), P(up_x), P(v["x_line"]), P(packet), P(o["gline"][1]), P(o["out"][1]),
                                               P(tab), *ext, plan.n_join_tiles, 1, 3, HB.FOLLOW, st) == 0
        assert lib.trunet_stream_highband_commit(P(v["x_line"]), P(packet), P(v["lo_line"]), P(x16), P(v["halo"]),
                                                 P(o["paired"][1]), P(ys16), P(v["energy"]), P(o["eline"][1]), P(v["gain"]),
                                                 P(o["gline"][1]), P(tab), *ext, HB.FOLLOW, st) == 0
        torch.cuda.synchronize()
        for full, view in o.values():
            assert (full[:pad] == SENTINEL).all() and (full[pad + view.shape[0]:] == SENTINEL).all()
        for k, t in s.items():
            assert (t[0] == SENTINEL).all() and (t[S + 1] == SENTINEL).all(), k
        return s, {k: view for k, (_, view) in o.items()}

    T = plan.table
    seg = lambda c_off, c_n, i, w=0: slice(int(T[i, c_off]) + w * i, int(T[i, c_off]) + w * i + int(T[i, c_n]) + w)
    good_s, good = call(T)
    for i in range(3):                                                 # the good run wrote every entry of every session
        assert not (good["out"][seg(4, 5, i)] == SENTINEL).any() and not (good["paired"][seg(9, 10, i)] == SENTINEL).any()
        assert not (good["gline"][seg(17, 13, i, 2)] == SENTINEL).any()
        assert not torch.equal(good_s["x_line"][1 + i], state0["x_line"][1 + i])
        assert not torch.equal(good_s["halo"][1 + i], state0["halo"][1 + i])
    # the lines after the commit: what was not consumed, then what came
    assert torch.equal(good_s["x_line"][2, :600], torch.cat([state0["x_line"][2, :700], packet[960:3460]])[2600:3200])
    assert torch.equal(good_s["lo_line"][2, :81], torch.cat([state0["lo_line"][2, :400], x16[320:1153]])[1152:1233])
    assert torch.equal(good["paired"][256:1408], torch.cat([state0["lo_line"][2, :400], x16[320:1153]])[:1152])

    big = 2 ** 41
    cases = [(0, S), (0, -1), (1, xcap + 1), (1, -1), (2, -1), (2, plan.n_packet - 2499), (3, -1), (3, plan.n_packet + 1),
             (4, -1), (4, plan.n_up - 2599), (5, -1), (5, plan.n_up + 1), (5, 700 + 2500 + 1), (6, -1), (6, SH.LO_LINE + 1),
             (7, -1), (7, plan.n_x16 - 832), (8, -1), (8, plan.n_x16 + 1), (9, -1), (9, plan.n_paired - 1151), (10, -1),
             (10, 1152 + 128), (10, 1151), (11, -1), (11, big), (12, -1), (12, big), (13, 8), (13, 10), (13, -1), (15, 2), (15, -1),
             (14, plan.n_join_tiles + 1), (16, plan.n_pair_tiles + 1), (17, plan.n_blocks - 8),
             (3, 100), (8, 100)]                                       # a packet too short for its outputs, x16 for its pairs
    for col, value in cases:
        tab = T.copy()
        tab[1, col] = value
        s, o = call(tab)
        what = (col, value)
        if col in (14, 16):                                            # a tile column is its own kernel's: the join's, the pairing's
            skipped = o["out"][seg(4, 5, 1)] if col == 14 else o["paired"][seg(9, 10, 1)]
            assert (skipped == SENTINEL).all(), what
        else:                                                          # every kernel skipped the record, the commit too
            assert (o["out"][seg(4, 5, 1)] == SENTINEL).all() and (o["paired"][seg(9, 10, 1)] == SENTINEL).all(), what
            assert (o["gline"][seg(17, 13, 1, 2)] == SENTINEL).all(), what
            assert (o["eline"].view(-1, 2)[seg(17, 13, 1, 3)] == SENTINEL).all(), what
            for k in state0:
                assert torch.equal(s[k][2], state0[k][2]), (what, k)
        assert torch.equal(o["out"][seg(4, 5, 0)], good["out"][seg(4, 5, 0)]), what
        for k in state0:
            assert torch.equal(s[k][1], good_s[k][1]), (what, k)
        if col not in (14, 16, 17):                                    # the last session's tiles and entries follow the changed record
            assert torch.equal(o["out"][seg(4, 5, 2)], good["out"][seg(4, 5, 2)]), what
            assert torch.equal(s["x_line"][3], good_s["x_line"][3]) and torch.equal(s["gain"][3], good_s["gain"][3]), what
