"""GPU: StreamPool.feed (tinyrecurrentunet_amd/streaming.py) -- packets of any size, many hops per call.  However an utterance
is cut into packets, the session must be bit for bit the step / close(tails) session of the same samples, and with that the
offline enhancement at the bounds of tests/test_stream_pool_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HOP = 128
LENS = [257, 384, 385, 1152, 513, 704, 1023, 1281, 258, 511, 832, 1407]
KINDS = ["fp32", "fp32-c3", "tgru", "int8"]


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


_NETS = {}


def _net(cin, use_tgru=False, seed=3):
    from oracle import network_ref as nr, weights as W
    from tinyrecurrentunet_amd import network as hn
    key = (cin, use_tgru, seed)
    if key not in _NETS:
        ref = W.fill_state_dict(nr.TRUNet(input_size=cin), seed=seed)
        net = hn.TRUNet(input_size=cin, use_tgru=use_tgru)
        net.load_state_dict(ref.state_dict())
        _NETS[key] = net.cuda().eval()
    return _NETS[key]


# kind -> (net, pool keywords, offline reference of a list of utterances, check of one session against it)
def _kind(kind):
    if kind in ("fp32", "fp32-c3"):
        net = _net(3 if kind == "fp32-c3" else 4)
        return net, {}, (lambda xs: net.enhance(xs)), (lambda y, r: _rel(y, r) < 1e-5)
    if kind == "tgru":
        net = _net(4, use_tgru=True, seed=5)
        return net, {}, (lambda xs: net.enhance(xs)), (lambda y, r: _rel(y, r) < 1e-4)
    assert kind == "int8"
    net = _net(4)
    return (net, {"int8": True}, (lambda xs: net.enhance(xs, path="int8")),
            (lambda y, r: float((y - r).abs().max()) <= 1e-2 * float(r.abs().max())))


def _audio(lens, seed=11, scale=0.1):
    g = np.random.default_rng(seed)
    return [torch.tensor(g.standard_normal(n) * scale, dtype=torch.float32).cuda() for n in lens]


def _by_steps(pool, x, slot=None):
    """the reference route: one step per whole hop, close with the tail"""
    s = pool.open(1)[0] if slot is None else slot
    outs = []
    for a in range(pool.hops(s), x.shape[0] // HOP):
        out, valid = pool.step(x[None, HOP * a:HOP * (a + 1)], [s])
        if valid[0]:
            outs.append(out[0])
    tail = x[HOP * (x.shape[0] // HOP):]
    return torch.cat(outs + pool.close([s], [tail if tail.shape[0] else None]))


def _cut(n, sizes):
    """packet lengths that add up to n: the sizes in turn (the last one repeated), the final packet cut short"""
    out, i = [], 0
    while n > 0 or not out:
        m = min(n, sizes[min(i, len(sizes) - 1)])
        out.append(m)
        n -= m
        i += 1
        assert i < 100000
    return out


def _check_call(pool, ids, before, lens, outs):
    """contract item 2 for one feed call"""
    for s, (a0, r0), n, o in zip(ids, before, lens, outs):
        a1, r1 = (HOP * a0 + r0 + n) // HOP, (r0 + n) % HOP
        assert o.dim() == 1 and o.shape[0] == HOP * (max(a1 - 3, 0) - max(a0 - 3, 0)), (s, a0, r0, n, o.shape)
        assert (pool.hops(s), pool.pending(s)) == (a1, r1)


def _feed_all(pool, xs, cuts, presteps=0, packed=False):
    """Every utterance through the pool by feed: sessions open while slots are free, every open session brings its next packet
    in one call, finished sessions close (without tails) in one call.  presteps: whole hops that go through step first."""
    n = len(xs)
    got, slot, at, pk = [[] for _ in xs], {}, [0] * n, [0] * n
    waiting, done = list(range(n)), 0
    while done < n:
        while waiting and pool.free:
            i = waiting.pop(0)
            (slot[i],) = pool.open(1)
            for a in range(min(presteps, xs[i].shape[0] // HOP)):
                out, valid = pool.step(xs[i][None, HOP * a:HOP * (a + 1)], [slot[i]])
                if valid[0]:
                    got[i].append(out[0])
                at[i] += HOP
            if presteps:
                cuts[i] = _cut(xs[i].shape[0] - at[i], [160])
        live = [i for i in sorted(slot) if pk[i] < len(cuts[i])]
        if live:
            ids = [slot[i] for i in live]
            lens = [cuts[i][pk[i]] for i in live]
            parts = [xs[i][at[i]:at[i] + m] for i, m in zip(live, lens)]
            before = [(pool.hops(s), pool.pending(s)) for s in ids]
            idle = {s: (pool.hops(s), pool.pending(s)) for i, s in slot.items() if i not in live}
            outs = pool.feed((torch.cat(parts), lens) if packed else parts, ids)
            assert len(outs) == len(ids)
            _check_call(pool, ids, before, lens, outs)
            assert all((pool.hops(s), pool.pending(s)) == v for s, v in idle.items())      # sitting the call out
            for i, m, o in zip(live, lens, outs):
                got[i].append(o)
                at[i] += m
                pk[i] += 1
        closing = [i for i in sorted(slot) if pk[i] >= len(cuts[i])]
        if closing:
            assert all(at[i] == xs[i].shape[0] for i in closing)
            for i, r in zip(closing, pool.close([slot[i] for i in closing])):
                got[i].append(r)
                del slot[i]
                done += 1
    return [torch.cat(g) for g in got]


def _random_cuts(xs, seed):
    g = np.random.default_rng(seed)
    cuts = []
    for x in xs:
        sizes = [int(v) for v in g.integers(0, 401, 40)]
        sizes[1], sizes[2], sizes[4] = 0, 1, 0                   # zeros and ones forced in
        cuts.append(_cut(x.shape[0], sizes + [400]))
    return cuts


# ---------------------------------------------------------------- 1. packetisation does not matter
@pytest.mark.parametrize("kind", KINDS)
def test_packetisation_does_not_matter_bit_for_bit(kind):
    """(i) step + close(tails), (ii) 160-sample packets, (iii) random packets of 0..400 samples with zeros and ones, (iv) one
    packet per utterance, (v) five hops by step and the rest by feed: every session the same bits, its own length, and the
    offline enhancement within the bound of its kind."""
    net, kw, offline, ok = _kind(kind)
    xs = _audio(LENS)
    pool = net.stream_pool(8, **kw)
    base = [_by_steps(pool, x) for x in xs]                                        # (i)
    runs = {"160": _feed_all(pool, xs, [_cut(x.shape[0], [160]) for x in xs]),
            "random": _feed_all(pool, xs, _random_cuts(xs, 21), packed=True),
            "whole": _feed_all(pool, xs, [[x.shape[0]] for x in xs]),
            "step5": _feed_all(pool, xs, [None] * len(xs), presteps=5)}
    assert pool.free == 8
    for name, got in runs.items():
        for x, y, b in zip(xs, got, base):
            assert y.shape == x.shape, (name, x.shape, y.shape)
            assert torch.equal(y, b), (kind, name, x.shape[0], _rel(y, b))
    refs = offline(xs)
    print("feed %s: worst vs offline %.3g" % (kind, max(_rel(y, r) for y, r in zip(base, refs))))
    for x, y, r in zip(xs, base, refs):
        assert ok(y, r), (kind, x.shape[0], _rel(y, r))


# ---------------------------------------------------------------- 2. independence
@pytest.mark.parametrize("kind", ["fp32", "tgru", "int8"])
def test_a_fed_session_does_not_depend_on_its_pool_mates(kind):
    net, kw, _, _ = _kind(kind)
    x, = _audio([1663], seed=4)
    cut = _cut(1663, [160, 5, 0, 400, 131])
    alone = _feed_all(net.stream_pool(1, **kw), [x], [cut])[0]
    mates = _audio([1500, 900, 1700], seed=6, scale=10.0)        # 100 times louder, other packet sizes
    for cap, order in ((4, [0, 1, 2, 3]), (4, [3, 1, 0, 2]), (16, [1, 2, 3, 0])):
        xs = [None] * 4
        cuts = [None] * 4
        for k, m in zip(order[1:], mates):
            xs[k], cuts[k] = m, _cut(m.shape[0], [97 + 64 * k, 300])
        xs[order[0]], cuts[order[0]] = x, cut
        pool = net.stream_pool(cap, **kw)
        if cap == 16:
            pool.open(5)                                         # five idle sessions: ours take slots 5.. of the larger pool
        got = _feed_all(pool, xs, cuts)[order[0]]
        assert torch.equal(got, alone), (kind, cap, order)


# ---------------------------------------------------------------- 3. lengths and latency
def test_lengths_hops_and_pending_after_every_call():
    net, kw, offline, ok = _kind("fp32")
    pool = net.stream_pool(3)
    a, b, c = pool.open(3)
    xa, xb, xc = _audio([128 * 10 + 57, 700, 300], seed=8)
    # one call takes a from 0 to 10 hops; b brings nothing; c sits the call out
    outs = pool.feed([xa[:1280], xb[:0]], [a, b])
    assert [o.shape[0] for o in outs] == [HOP * 7, 0]
    assert (pool.hops(a), pool.pending(a), pool.hops(b), pool.pending(b), pool.hops(c), pool.pending(c)) == (10, 0, 0, 0, 0, 0)
    ya = [outs[0]]
    # the call's sequence of (packet of a, packet of b, packet of c); None: the session sits the call out
    sched = [(0, 383, None), (None, 1, 300), (57, 0, None), (None, 316, 0)]
    at = {a: 1280, b: 0, c: 0}
    got = {a: ya, b: [], c: []}
    src = {a: xa, b: xb, c: xc}
    for call in sched:
        ids = [s for s, m in zip((a, b, c), call) if m is not None]
        lens = [m for m in call if m is not None]
        before = [(pool.hops(s), pool.pending(s)) for s in ids]
        outs = pool.feed([src[s][at[s]:at[s] + m] for s, m in zip(ids, lens)], torch.tensor(ids))
        _check_call(pool, ids, before, lens, outs)
        for s, m, o in zip(ids, lens, outs):
            got[s].append(o)
            at[s] += m
    assert (pool.hops(b), pool.pending(b)) == (5, 60) and (pool.hops(c), pool.pending(c)) == (2, 44)
    rest = pool.close([a, b, c])
    assert pool.free == 3
    refs = offline([xa, xb, xc])
    for s, r, ref in zip((a, b, c), rest, refs):
        y = torch.cat(got[s] + [r])
        assert y.shape == src[s].shape and ok(y, ref)
    assert pool.feed([], []) == []


# ---------------------------------------------------------------- 4. misuse
def test_feed_misuse_raises_and_leaves_the_sessions_alone():
    net, kw, _, _ = _kind("fp32")
    X = _audio([HOP * 12 + 40, HOP * 12 + 40], seed=9)
    ref = net.stream_pool(2)
    want = [_by_steps(ref, X[0]), _by_steps(ref, X[1])]
    pool = net.stream_pool(4)
    ids = pool.open(2)
    idle = 3
    outs = [[], []]
    at = [0]

    def feed(m):
        for j, o in enumerate(pool.feed([X[0][at[0]:at[0] + m], X[1][at[0]:at[0] + m]], ids)):
            outs[j].append(o)
        at[0] += m

    def refused(fn, *a, **k):
        state = (list(pool._hops), list(pool._pend), pool.free)
        with pytest.raises(Exception) as e:
            fn(*a, **k)
        assert not isinstance(e.value, (AssertionError, AttributeError, TypeError, IndexError)), repr(e.value)
        assert (list(pool._hops), list(pool._pend), pool.free) == state

    feed(700)                                                    # 5 hops, 60 pending
    assert pool.pending(ids[0]) == 60
    p = [X[0][:50], X[1][:50]]
    c = torch.stack([X[0][:HOP], X[1][:HOP]])
    refused(pool.step, c, ids)                                   # step with pending samples
    refused(pool.close, ids, [X[0][:5], None])                   # a tail on top of pending samples
    refused(pool.close, ids, [None, X[0][:0]])
    refused(pool.feed, [t.cpu() for t in p], ids)                # packets on the CPU
    refused(pool.feed, [p[0], p[1].cpu()], ids)
    refused(pool.feed, [p[0][None], p[1][None]], ids)            # 2-D packets
    refused(pool.feed, torch.stack(p), ids)
    refused(pool.feed, [p[0], p[1].long()], ids)
    refused(pool.feed, p, torch.tensor(ids).cuda())              # device ids
    refused(pool.feed, p, [ids[0], 99])                          # unknown
    refused(pool.feed, p, [ids[0], -1])
    refused(pool.feed, p, [ids[0], idle])                        # idle
    refused(pool.feed, p, [ids[0], ids[0]])                      # repeated
    refused(pool.feed, p[:1], ids)                               # one packet for two sessions
    refused(pool.feed, (torch.cat(p), [50, 49]), ids)            # packed: lengths do not add up
    refused(pool.feed, (torch.cat(p), [101, -1]), ids)
    refused(pool.feed, (torch.cat(p), [100]), ids)
    refused(pool.feed, (torch.cat(p).cpu(), [50, 50]), ids)
    refused(pool.pending, idle)
    feed(68)                                                     # 6 hops, nothing pending: step is allowed again
    assert pool.pending(ids[0]) == 0
    out, valid = pool.step(torch.stack([X[0][at[0]:at[0] + HOP], X[1][at[0]:at[0] + HOP]]), ids)
    assert valid.tolist() == [True, True]
    outs[0].append(out[0])
    outs[1].append(out[1])
    at[0] += HOP
    (short,) = pool.open(1)
    assert pool.feed([X[0][:256]], [short])[0].shape[0] == 0
    refused(pool.close, [short])                                 # a fed session of 256 samples
    refused(pool.close, [ids[0], short])                         # ... and the long session of the same call stays open
    pool.feed([X[0][256:257]], [short])
    (r,) = pool.close([short])
    assert r.shape == (257,)
    feed(X[0].shape[0] - at[0])
    rest = pool.close(ids)
    for j in range(2):
        assert torch.equal(torch.cat(outs[j] + [rest[j]]), want[j]), j


# ---------------------------------------------------------------- 5. slot re-use
@pytest.mark.parametrize("kind", ["fp32", "tgru"])
def test_pending_samples_do_not_reach_the_next_session_in_the_slot(kind):
    net, kw, _, _ = _kind(kind)
    loud, quiet = _audio([2000], seed=77, scale=5.0)[0], _audio([1577], seed=78)[0]
    cut = _cut(1577, [100, 333])
    fresh = _feed_all(net.stream_pool(1, **kw), [quiet], [cut])[0]
    pool = net.stream_pool(1, **kw)
    _feed_all(pool, [loud], [_cut(2000, [333])])                 # closed with 80 pending samples
    assert torch.equal(_feed_all(pool, [quiet], [cut])[0], fresh)
    for stop in (1500, 200, 100):                                # aborted with pending samples: steady, collecting, first packet
        (s,) = pool.open(1)
        pool.feed([loud[:stop]], [s])
        assert pool.pending(s) == stop % HOP != 0
        pool.abort([s])
        assert torch.equal(_feed_all(pool, [quiet], [cut])[0], fresh), stop
    (s,) = pool.open(1)                                          # ... and a step session after a fed one
    pool.feed([loud[:777]], [s])
    pool.abort([s])
    assert torch.equal(_by_steps(pool, quiet), fresh)


# ---------------------------------------------------------------- 6. bursts and slicing of the network stage
@pytest.mark.parametrize("kind", ["fp32", "tgru"])
def test_bursts_and_network_slices(kind):
    net, kw, offline, ok = _kind(kind)
    xs = _audio([48000, 48000, 47999, 48001], seed=31)
    refs = offline(xs)
    whole = _feed_all(net.stream_pool(4, **kw), xs, [[x.shape[0]] for x in xs])
    assert "fold_max_frames" not in vars(net)
    net.fold_max_frames = 256
    try:
        sliced = _feed_all(net.stream_pool(4, **kw), xs, [[x.shape[0]] for x in xs])
    finally:
        del net.fold_max_frames
    assert net.fold_max_frames == type(net).fold_max_frames
    for x, y, z, r in zip(xs, whole, sliced, refs):
        assert y.shape == x.shape and torch.equal(y, z)
        assert ok(y, r), (kind, _rel(y, r))
    assert torch.equal(whole[2], _by_steps(net.stream_pool(1, **kw), xs[2]))


# ---------------------------------------------------------------- 7. entry points
def test_feed_entry_points_skip_records_outside_the_extents():
    from tinyrecurrentunet_amd import _lib as L, streaming as sm
    from tinyrecurrentunet_amd._lib import ptr
    lib, st, p = L.lib(), L.stream(), sm.PCEN
    CAN, S16, S8, E, FI = 7.5, 16, 8, L.TRUNET_EINVAL, sm.FEED_INTS
    can = lambda *s: torch.full(s, CAN, device="cuda", dtype=torch.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tw = L.twiddles(512, torch.device("cuda"))
    g = torch.Generator(device="cuda").manual_seed(3)
    pc = (p["eps"], p["s"], p["alpha"], p["delta"], p["r"])
    rnd = lambda *s: torch.randn(s, device="cuda", generator=g) * 0.1
    ring0, fifo0, M0, ola0 = rnd(S16, 512), rnd(S16, 128), rnd(S16, 257).abs() + 0.1, rnd(S16, 512)
    hops, pend = np.full(S16, 4, np.int64), np.full(S16, 5, np.int64)
    hops[5] = 0                                                  # slot 5 starts: frames 0 and 1 in one record pair
    smp = rnd(1200)

    def front(plan, slots, rows=None, sess=None, seq=None, n_samples=None):
        rows = dev(plan.rows if rows is None else rows)
        sess, seq = dev(plan.sess if sess is None else sess), dev(plan.seq if seq is None else seq)
        n_rows, ns = len(plan.rows), plan.n_samples if n_samples is None else n_samples
        ring, fifo, M, feat = ring0.clone(), fifo0.clone(), M0.clone(), can(n_rows, 4, 257)
        ring[S8:], fifo[S8:], M[S8:] = CAN, CAN, CAN
        assert lib.trunet_stream_feed_features(ptr(ring), ptr(fifo), ptr(smp), ptr(feat), rows.data_ptr(), n_rows, ns, slots,
                                               ptr(tw), 4, st) == 0
        assert lib.trunet_stream_feed_commit(ptr(ring), ptr(fifo), ptr(smp), ptr(M), ptr(feat), rows.data_ptr(), sess.data_ptr(),
                                             seq.data_ptr(), len(plan.sess), n_rows, ns, slots, 4, *pc, st) == 0
        torch.cuda.synchronize()
        return ring, fifo, M, feat

    def back(plan, slots, frames, rows=None, n_out=None):
        rows, sess, seq = dev(plan.rows if rows is None else rows), dev(plan.sess), dev(plan.seq)
        n_out = plan.n_out if n_out is None else n_out
        ola, out = ola0.clone(), can(plan.n_out, 128)
        ola[S8:] = CAN
        assert lib.trunet_stream_feed_ola(ptr(frames), ptr(ola), ptr(out), rows.data_ptr(), sess.data_ptr(), seq.data_ptr(),
                                          plan.n_active, len(plan.rows), n_out, slots, st) == 0
        torch.cuda.synchronize()
        return ola, out

    def of(plan, k):
        """frame records and out hops of the session at position k of the call"""
        (s,) = [v for v in plan.sess if v[9] == k]
        rows = plan.seq[s[2]:s[2] + s[3]]
        return rows, [int(plan.rows[i, 8]) for i in rows if plan.rows[i, 8] >= 0]

    lens = [300, 400, 500]
    bad = sm.plan_feed(hops, pend, lens, [3, 8, 5])              # slot 8 is outside the 8 declared slots
    good = sm.plan_feed(hops, pend, [300, 500], [3, 5])
    good.rows[:, 6] += np.where(good.rows[:, 0] == 5, 400, 0)    # the same samples as in the call of three
    good.sess[:, 7] += np.where(good.sess[:, 0] == 5, 400, 0)
    goodp = good._replace(n_samples=1200)
    ring_w, fifo_w, M_w, feat_w = front(goodp, S16)
    untouched = [s for s in range(S8) if s not in (3, 5)]

    # ---- refusals launch nothing
    rows, sess, seq = dev(bad.rows), dev(bad.sess), dev(bad.seq)
    ring, fifo, M, feat, frames, ola, out = can(S16, 512), can(S16, 128), can(S16, 257), can(len(bad.rows), 4, 257), \
        can(len(bad.rows), 512), can(S16, 512), can(bad.n_out, 128)
    y = torch.randn((len(bad.rows), 8, 257), device="cuda", generator=g)
    n_rows = len(bad.rows)
    assert lib.trunet_stream_feed_features(ptr(ring), ptr(fifo), None, ptr(feat), rows.data_ptr(), n_rows, 1200, S8, ptr(tw),
                                           4, st) == E
    assert lib.trunet_stream_feed_features(ptr(ring), ptr(fifo), ptr(smp), ptr(feat), rows.data_ptr(), 0, 1200, S8, ptr(tw),
                                           4, st) == E
    assert lib.trunet_stream_feed_features(ptr(ring), ptr(fifo), ptr(smp), ptr(feat), rows.data_ptr(), n_rows, 1200, S8,
                                           ptr(tw), 5, st) == E
    assert lib.trunet_stream_feed_commit(ptr(ring), ptr(fifo), ptr(smp), None, ptr(feat), rows.data_ptr(), sess.data_ptr(),
                                         seq.data_ptr(), 3, n_rows, 1200, S8, 4, *pc, st) == E
    assert lib.trunet_stream_feed_commit(ptr(ring), ptr(fifo), ptr(smp), ptr(M), ptr(feat), rows.data_ptr(), sess.data_ptr(),
                                         seq.data_ptr(), 3, n_rows, -1, S8, 4, *pc, st) == E
    assert lib.trunet_stream_feed_mask_istft(ptr(y), ptr(frames), 0, ptr(tw), 0.5, st) == E
    assert lib.trunet_stream_feed_mask_istft(ptr(y), None, n_rows, ptr(tw), 0.5, st) == E
    assert lib.trunet_stream_feed_ola(ptr(frames), ptr(ola), None, rows.data_ptr(), sess.data_ptr(), seq.data_ptr(), 3, n_rows,
                                      bad.n_out, S8, st) == E
    assert lib.trunet_stream_feed_ola(ptr(frames), ptr(ola), ptr(out), rows.data_ptr(), sess.data_ptr(), seq.data_ptr(), 3,
                                      n_rows, bad.n_out, 0, st) == E
    torch.cuda.synchronize()
    for t in (ring, fifo, M, feat, frames, ola, out):
        assert bool((t == CAN).all())

    # ---- front end: the records of slot 8 are skipped, slots 3 and 5 come out as in a call without it
    def check_front(res, plan, skipped, same):
        ring, fifo, M, feat = res
        assert bool((ring[S8:] == CAN).all()) and bool((fifo[S8:] == CAN).all()) and bool((M[S8:] == CAN).all())
        for k in skipped:
            slot = int([v for v in plan.sess if v[9] == k][0][0])
            assert bool((feat[of(plan, k)[0]] == CAN).all())
            if slot < S8:
                assert torch.equal(ring[slot], ring0[slot]) and torch.equal(fifo[slot], fifo0[slot])
                assert torch.equal(M[slot], M0[slot])
        for k, kw_ in same:
            slot = int([v for v in plan.sess if v[9] == k][0][0])
            assert torch.equal(feat[of(plan, k)[0]], feat_w[of(good, kw_)[0]])
            assert torch.equal(ring[slot], ring_w[slot]) and torch.equal(fifo[slot], fifo_w[slot])
            assert torch.equal(M[slot], M_w[slot])
        assert torch.equal(ring[untouched], ring0[untouched]) and torch.equal(fifo[untouched], fifo0[untouched])
        assert torch.equal(M[untouched], M0[untouched])

    check_front(front(bad, S8), bad, [1], [(0, 0), (2, 1)])
    # the ring moved on by the whole hops, the FIFO holds what is left (slot 3: 5 + 300 = 2 hops + 49)
    line = torch.cat([ring0[3], fifo0[3, :5], smp[:300]])
    assert torch.equal(ring_w[3], line[256:768]) and torch.equal(fifo_w[3, :49], line[768:817])
    assert torch.equal(fifo_w[3, 49:], fifo0[3, 49:])
    # sample range outside the packed samples: the session of slot 3 claims 300 samples from 1000 of 1200 declared
    rows_, sess_ = bad.rows.copy(), bad.sess.copy()
    rows_[rows_[:, 0] == 3, 6] = 1000
    sess_[sess_[:, 0] == 3, 7] = 1000
    check_front(front(bad, S8, rows=rows_, sess=sess_), bad, [0, 1], [(2, 1)])
    check_front(front(bad, S8, n_samples=899), bad, [1, 2], [(0, 0)])          # slot 5's packet ends at 1200
    # a window that leaves the line, a pair row and a frame list outside the feature rows
    rows_ = bad.rows.copy()
    rows_[(rows_[:, 0] == 3) & (rows_[:, 2] == 4), 3] = 5 + 300 + 1
    res = front(bad, S8, rows=rows_)
    i4 = [i for i in of(bad, 0)[0] if bad.rows[i, 2] == 4]
    assert bool((res[3][i4][:, [0, 2, 3]] == CAN).all())          # (channel 1 of the row still goes through the PCEN stage)
    rows_ = bad.rows.copy()
    rows_[(rows_[:, 0] == 5) & (rows_[:, 9] >= 0), 9] = n_rows
    res = front(bad, S8, rows=rows_)
    first = [i for i in of(bad, 2)[0] if bad.rows[i, 2] <= 1]
    assert bool((res[3][first][:, [0, 2, 3]] == CAN).all())
    seq_ = bad.seq.copy()
    seq_[int([v for v in bad.sess if v[9] == 0][0][2])] = n_rows
    check_front(front(bad, S8, seq=seq_), bad, [1], [(2, 1)])
    res = front(bad, S8, seq=seq_)
    assert torch.equal(res[0][3], ring0[3]) and torch.equal(res[2][3], M0[3])  # the session with the bad list: no commit

    # ---- back end
    y_w = torch.randn((len(good.rows), 8, 257), device="cuda", generator=g)
    fr_w = can(len(good.rows), 512)
    assert lib.trunet_stream_feed_mask_istft(ptr(y_w), ptr(fr_w), len(good.rows), ptr(tw), 0.5, st) == 0
    ola_w, out_w = back(good, S16, fr_w)
    assert not bool((out_w == CAN).any())
    fr = rnd(n_rows, 512)
    for k, kw_ in ((0, 0), (2, 1)):
        fr[of(bad, k)[0]] = fr_w[of(good, kw_)[0]]
    ola, out = back(bad, S8, fr)
    assert bool((ola[S8:] == CAN).all()) and bool((out[of(bad, 1)[1]] == CAN).all())
    for k, kw_ in ((0, 0), (2, 1)):
        slot = (3, 8, 5)[k]
        assert torch.equal(out[of(bad, k)[1]], out_w[of(good, kw_)[1]]) and torch.equal(ola[slot], ola_w[slot])
    assert torch.equal(ola[untouched], ola0[untouched])
    # an out hop outside n_out: the whole session is skipped, the other one is not
    rows_ = bad.rows.copy()
    last = of(bad, 0)[0][-1]
    rows_[last, 8] = bad.n_out
    ola, out = back(bad, S8, fr, rows=rows_)
    assert bool((out[of(bad, 0)[1]] == CAN).all()) and torch.equal(ola[3], ola0[3])
    assert torch.equal(out[of(bad, 2)[1]], out_w[of(good, 1)[1]]) and torch.equal(ola[5], ola_w[5])
    ola, out = back(bad, S8, fr, n_out=1)                        # slot 3 owns hops 0 and 1: hop 1 is outside an output of one hop
    assert of(bad, 0)[1] == [0, 1] and bool((out == CAN).all()) and torch.equal(ola[3], ola0[3])
    assert torch.equal(ola[5], ola_w[5])
