"""GPU: the attenuation limit (tinyrecurrentunet_amd/atten.py, csrc/atten.hip) on every route: enhance,
AudioStream and the stream pool, at 16 kHz and above.

The bounds are derived, not measured.  The blend out = y + g (x - y) is two or three fp32 roundings of quantities no larger
than |x| + |y|: a limited output lies within 4 * 2^-24 (|x| + |y|) of the float64 value computed from x, the fp32 g and the
SAME route's unlimited output y (a separate call: existing code); inside the hop over which a limit moves the fp32 rounding
of the ramp's gain adds as much again, 8 * 2^-24.  The blend is a convex combination for g in [0, 1], so two limited routes
may differ by what the unlimited ones may: the pool against enhance at the bounds of DESIGN section 3g."""
import numpy as np
import pytest
import torch

import atten_ref as AR
import highband_ref as HR
import stream_highband_ref as SR

pytestmark = pytest.mark.gpu

HOP = 128
INF = float("inf")
U32 = 2.0 ** -24
LENS = [257, 383, 384, 385, 1152, 4000]
LIMS = [0.0, 6.0, 12.0, 20.0, 40.0, INF]
_NETS, _CHURN = {}, {}


def _net(cin, use_tgru=False):
    from oracle import network_ref as nr, weights as W
    from tinyrecurrentunet_amd import network as hn
    key = (cin, use_tgru)
    if key not in _NETS:
        net = hn.TRUNet(input_size=cin, use_tgru=use_tgru)
        net.load_state_dict(W.fill_state_dict(nr.TRUNet(input_size=cin), seed=5).state_dict())
        _NETS[key] = net.cuda().eval()
    return _NETS[key]


def _audio(lens, seed=11, scale=0.1):
    g = np.random.default_rng(seed)
    return [torch.tensor(g.standard_normal(n) * scale, dtype=torch.float32).cuda() for n in lens]


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _check_blend(out, x, y, g, what, in_ramp=None):
    """|out - (y + g (x - y))| <= 4 * 2^-24 (|x| + |y|) sample by sample, 8 * 2^-24 where in_ramp; prints the largest ratio"""
    assert out.shape == x.shape == y.shape and out.dtype == torch.float32, (what, out.shape, x.shape, y.shape)
    o, x, y = _np(out), _np(x), _np(y)
    bound = AR.bound(x, y) if in_ramp is None else np.where(in_ramp, AR.bound(x, y, 8), AR.bound(x, y, 4))
    err = np.abs(o - AR.blend(x, y, g))
    ratio = float(np.max(err / np.maximum(bound, 1e-300)))
    print("%s: largest |err| / bound = %.3f" % (what, ratio))
    assert np.all(err <= bound), (what, ratio, int(np.argmax(err / np.maximum(bound, 1e-300))))


# ---------------------------------------------------------------- 5. offline: the formula
OFFLINE = [(3, False, "folded"), (3, False, "layers"), (4, False, "folded"), (4, False, "layers"), (4, False, "int8"),
           (4, True, "auto")]


@pytest.mark.parametrize("cin,tgru,path", OFFLINE)
def test_enhance_with_a_limit_is_the_blend_of_its_own_result(cin, tgru, path):
    from tinyrecurrentunet_amd.enhance import enhance
    net = _net(cin, tgru)
    xs = _audio(LENS)
    ys = enhance(net, xs, path=path)                                       # a call without the keyword
    none = enhance(net, xs, path=path, atten_lim_db=None)
    outs = enhance(net, xs, path=path, atten_lim_db=LIMS)
    for x, y, n, o, L in zip(xs, ys, none, outs, LIMS):
        assert torch.equal(n, y)
        _check_blend(o, x, y, AR.gain(L), "enhance %s C_in %d L %d at %g dB" % (path, cin, x.shape[0], L))
    assert torch.equal(outs[5], ys[5])                                     # inf: the unlimited result bit for bit
    assert np.all(np.abs(_np(outs[0]) - _np(xs[0])) <= AR.bound(_np(xs[0]), _np(ys[0])))      # 0 dB: the input, within the bound
    assert not torch.equal(outs[1], ys[1])
    # a tensor of limits: the same bits
    for o, t in zip(outs, enhance(net, xs, path=path, atten_lim_db=torch.tensor(LIMS))):
        assert torch.equal(o, t)
    if path != "folded":
        return
    # a scalar, another batch, the padded form: the same bits
    twelve = enhance(net, [xs[4], xs[2]], path=path, atten_lim_db=12.0)
    assert torch.equal(twelve[1], outs[2])
    X = torch.zeros((2, 1200), device="cuda")
    X[0, :1152], X[1, :384] = xs[4], xs[2]
    Y = enhance(net, X, lengths=[1152, 384], path=path, atten_lim_db=[12.0, 12.0])
    assert torch.equal(Y[0, :1152], twelve[0]) and torch.equal(Y[1, :384], twelve[1]) and not Y[0, 1152:].any()


# ---------------------------------------------------------------- 6. offline at 48 kHz: the limit sits inside the 16 kHz stage
@pytest.mark.parametrize("mode", ["drop", "keep", "follow"])
def test_enhance_at_48_khz_is_the_composition_with_the_limit_at_16_khz(mode):
    from tinyrecurrentunet_amd import highband as HB, resample as R
    from tinyrecurrentunet_amd.enhance import enhance
    net, fs = _net(4), 48000
    xs = _audio([771, 772, 3001, 12007], seed=12)
    lims = [6.0, 20.0, INF, 0.0]
    got = enhance(net, xs, fs=fs, highband=mode, highband_floor_db=-40.0, atten_lim_db=lims)
    down = R.resample(xs, fs, 16000)
    den = enhance(net, down, atten_lim_db=lims)
    up = R.resample(den, 16000, fs) if mode == "drop" else HB.rejoin(xs, down, den, fs, mode, -40.0)
    plain = enhance(net, xs, fs=fs, highband=mode, highband_floor_db=-40.0)
    for x, y, u, p, L in zip(xs, got, up, plain, lims):
        assert y.shape == x.shape and torch.equal(y, u[:x.shape[0]]), (mode, x.shape[0])
        assert torch.equal(y, p) == (L == INF), (mode, L)


# ---------------------------------------------------------------- the pool: sessions that come and go, each with its limit
# (samples, route, limit in dB, amplitude): "feed" sessions arrive in packets of one size, "step" sessions in hops and end
# with a tail of 1, 64 or 127 samples.  Nine sessions on four slots: every slot is used again.
SESSIONS = [(257, ("feed", 1), 6.0, 0.1), (383, ("feed", 127), 12.0, 0.1), (384, ("feed", 128), 0.0, 1.0),
            (385, ("feed", 129), 20.0, 0.1), (1152, ("feed", 160), 40.0, 1.0), (4000, ("feed", 1000), INF, 0.1),
            (4 * HOP + 1, ("step", 1), 3.0, 0.1), (2 * HOP + 64, ("step", 64), 12.0, 1.0), (9 * HOP + 127, ("step", 127), 6.0, 0.1)]
KINDS = {"c4": (4, False, False), "c3": (3, False, False), "tgru": (4, True, False), "int8": (4, False, True)}


def _session_audio():
    return [_audio([n], seed=3 * n + 1, scale=s)[0] for n, _, _, s in SESSIONS]


def _pool(kind, slots, **kw):
    cin, tgru, int8 = KINDS[kind]
    return _net(cin, tgru).stream_pool(slots, int8=int8, **kw)


def _churn(pool, xs, lims, only=None):
    """Every session of SESSIONS (or those in ``only``) through ``pool``: a session opens when a slot is free and is given
    its limit (lims None: a pool without limits), sits out every fifth round counted from its own opening, brings its next
    packet or hop otherwise -- all feeds of a round in one call, all steps in another -- and closes, with the others of its
    round, when its samples are through.  -> the sessions' outputs."""
    todo = list(range(len(SESSIONS))) if only is None else list(only)
    got, slot, at, born = {i: [] for i in todo}, {}, {}, {}
    rnd = 0
    while todo or slot:
        while todo and pool.free:
            i = todo.pop(0)
            (slot[i],) = pool.open(1)
            at[i], born[i] = 0, rnd
            if lims is not None:
                pool.set_atten_lim([slot[i]], lims[i])
        live = [i for i in sorted(slot) if (rnd - born[i]) % 5 != 4]
        feeds = [i for i in live if SESSIONS[i][1][0] == "feed" and at[i] < xs[i].shape[0]]
        if feeds:
            parts = [xs[i][at[i]:at[i] + SESSIONS[i][1][1]] for i in feeds]
            for i, p, o in zip(feeds, parts, pool.feed(parts, [slot[i] for i in feeds])):
                got[i].append(o)
                at[i] += p.shape[0]
        steps = [i for i in live if SESSIONS[i][1][0] == "step" and at[i] + HOP <= xs[i].shape[0]]
        if steps:
            out, valid = pool.step(torch.stack([xs[i][at[i]:at[i] + HOP] for i in steps]), [slot[i] for i in steps])
            for k, i in enumerate(steps):
                if valid[k]:
                    got[i].append(out[k])
                at[i] += HOP
        done = [i for i in live if xs[i].shape[0] - at[i] < (HOP if SESSIONS[i][1][0] == "step" else 1)]
        if done:
            tails = [xs[i][at[i]:] if SESSIONS[i][1][0] == "step" else None for i in done]
            for i, r in zip(done, pool.close([slot[i] for i in done], tails)):
                got[i].append(r)
                del slot[i]
        rnd += 1
        assert rnd < 5000
    return {i: torch.cat(v) for i, v in got.items()}


def _churn_run(kind, limited):
    key = (kind, limited)
    if key not in _CHURN:
        xs = _session_audio()
        lims = [L for _, _, L, _ in SESSIONS]
        pool = _pool(kind, 4, atten_lim_db=30.0) if limited else _pool(kind, 4)
        res = _churn(pool, xs, lims if limited else None)
        assert pool.free == 4 and all(res[i].shape == x.shape for i, x in enumerate(xs))
        _CHURN[key] = res
    return _CHURN[key]


# ---------------------------------------------------------------- 7. the pool against enhance, both with the limit
@pytest.mark.parametrize("kind", ["c4", "c3", "tgru", "int8"])
def test_pool_sessions_with_limits_against_enhance_with_the_same_limits(kind):
    from tinyrecurrentunet_amd.enhance import enhance
    cin, tgru, int8 = KINDS[kind]
    xs, res = _session_audio(), _churn_run(kind, True)
    refs = enhance(_net(cin, tgru), xs, path="int8" if int8 else "auto", atten_lim_db=[L for _, _, L, _ in SESSIONS])
    for i, (x, r) in enumerate(zip(xs, refs)):
        y = res[i]
        print("pool %s, session %d (%d samples, %g dB): %.3g of the peak" % (kind, i, x.shape[0], SESSIONS[i][2], _rel(y, r)))
        if int8:
            assert float((y - r).abs().max()) <= 1e-2 * float(r.abs().max()), (i, _rel(y, r))
        else:
            assert _rel(y, r) < (1e-4 if tgru else 1e-5), (i, _rel(y, r))


# ---------------------------------------------------------------- 8. the pool: the formula, against the pool without limits
@pytest.mark.parametrize("kind", ["c4", "tgru", "int8"])
def test_pool_with_limits_is_the_blend_of_the_pool_without(kind):
    xs, wet, res = _session_audio(), _churn_run(kind, False), _churn_run(kind, True)
    for i, x in enumerate(xs):
        L = SESSIONS[i][2]
        _check_blend(res[i], x, wet[i], AR.gain(L), "pool %s session %d (%d samples) at %g dB" % (kind, i, x.shape[0], L))
        assert torch.equal(res[i], wet[i]) == (L == INF), i
    # a pool whose limit is inf and is never moved: the pool without a limit, bit for bit
    same = _churn(_pool(kind, 4, atten_lim_db=INF), xs, None, only=[1, 4, 7, 8])
    for i, y in same.items():
        assert torch.equal(y, wet[i]), i


# ---------------------------------------------------------------- 9. the pool's guarantees hold with a limit
def _one(pool, x, L, cut=None, change=None):
    """one session alone: by steps and a tail (cut None), or by packets of ``cut`` samples (a list: those sizes, the last one
    repeated); change = (P, L_new): the limit moves when P samples have been fed (a packet boundary is made there)"""
    s, = pool.open(1)
    if L is not None:
        pool.set_atten_lim([s], L)
    n, at, outs = x.shape[0], 0, []
    sizes = [HOP] if cut is None else ([cut] if isinstance(cut, int) else list(cut))
    k = 0
    while True:
        if change is not None and at == change[0]:
            pool.set_atten_lim([s], change[1])
        m = min(sizes[min(k, len(sizes) - 1)], n - at)
        if change is not None and at < change[0]:
            m = min(m, change[0] - at)
        if cut is None:
            if m < HOP:
                break
            out, valid = pool.step(x[None, at:at + HOP], [s])
            if valid[0]:
                outs.append(out[0])
        else:
            if at >= n:
                break
            outs.append(pool.feed([x[at:at + m]], [s])[0])                 # m = 0: an empty packet
        at += m
        k += 1
    tail = x[at:] if cut is None and at < n else None
    return torch.cat(outs + pool.close([s], [tail]))


def test_packets_do_not_matter_with_a_limit():
    pool = _pool("c4", 2, atten_lim_db=9.0)
    for x, L in zip(_audio(LENS, seed=17), (None, 6.0, 20.0, 12.0, 3.0, 40.0)):
        base = _one(pool, x, L)                                            # step + close(tails)
        assert base.shape == x.shape
        for cut in ((1, 127, 129) if x.shape[0] <= 385 else (127, 129, 160, 1000, [5, 0, 300, 1, 700])):
            assert torch.equal(_one(pool, x, L, cut), base), (x.shape[0], cut)
    assert pool.free == 2


def test_a_limited_session_does_not_depend_on_its_pool_mates():
    """alone in a pool of one slot against the churn run, where the mates have other limits and some are 10 times louder"""
    xs, res = _session_audio(), _churn_run("c4", True)
    lims = [L for _, _, L, _ in SESSIONS]
    for i in (0, 3, 4, 6, 8):
        alone = _churn(_pool("c4", 1, atten_lim_db=30.0), xs, lims, only=[i])[i]
        assert torch.equal(alone, res[i]), i
    big = _pool("c4", 16, atten_lim_db=30.0)
    idle = big.open(5)                                                     # other slot ids, another capacity
    big.set_atten_lim(idle, [0.0, 1.0, 2.0, 3.0, INF])
    other = _churn(big, xs, lims, only=[8, 3, 1])
    for i, y in other.items():
        assert torch.equal(y, res[i]), i


# ---------------------------------------------------------------- 10. a limit that moves while the session runs
def _check_moved(out, x, wet, g_open, changes, what):
    g, in_ramp = AR.session_gains(x.shape[0], g_open, changes)
    assert in_ramp.sum() == HOP * sum(1 for P, _ in changes if P >= 3 * HOP)
    _check_blend(out, x, wet, g, what, in_ramp)


def test_a_limit_moved_between_two_steps():
    x, = _audio([12 * HOP + 64], seed=23)
    wet = _one(_pool("c4", 1), x, None)
    pool = _pool("c4", 1, atten_lim_db=20.0)
    out = _one(pool, x, None, None, (6 * HOP, 6.0))
    _check_moved(out, x, wet, AR.gain(20.0), [(6 * HOP, AR.gain(6.0))], "moved between steps")
    assert not torch.equal(out[3 * HOP:4 * HOP], _one(pool, x, 6.0)[3 * HOP:4 * HOP])      # the ramp is there
    # the same place by feed, cut two ways: the same bits
    for cut in (6 * HOP, [500, 268, 160]):
        assert torch.equal(_one(pool, x, None, cut, (6 * HOP, 6.0)), out), cut
    # twice in a session, the second time towards "no limit"; and a change before frame 0, which is no ramp
    out = _one(pool, x, None, None, (10 * HOP, INF))
    _check_moved(out, x, wet, AR.gain(20.0), [(10 * HOP, 0.0)], "moved to inf")
    assert torch.equal(out[8 * HOP:], wet[8 * HOP:])
    out = _one(pool, x, None, 160, (2 * HOP, 6.0))
    _check_moved(out, x, wet, AR.gain(20.0), [(2 * HOP, AR.gain(6.0))], "moved before frame 0")
    assert torch.equal(out, _one(pool, x, 6.0))


def test_a_limit_moved_between_two_feeds_that_split_a_hop():
    x, = _audio([1600], seed=29)
    wet = _one(_pool("c4", 1), x, None, 160)
    pool = _pool("c4", 2, atten_lim_db=12.0)
    out = _one(pool, x, None, [700, 333], (700, 40.0))                     # 5 hops and 60 samples are in: two hops are out
    _check_moved(out, x, wet, AR.gain(12.0), [(700, AR.gain(40.0))], "moved between feeds")
    for cut in ([300, 400, 1000], 127, [699, 1, 0, 1, 899]):                    # the call at the same sample, other packets
        assert torch.equal(_one(pool, x, None, cut, (700, 40.0)), out), cut
    # at the end of the input: the ramp lies in the first hop that close() returns
    out = _one(pool, x, None, 160, (1600, 0.0))
    _check_moved(out, x, wet, AR.gain(12.0), [(1600, 1.0)], "moved before close")


def test_a_reused_slot_starts_at_its_own_target():
    xa, xb = _audio([1400, 900], seed=31)
    pool = _pool("c4", 1, atten_lim_db=20.0)
    fresh = _one(pool, xb, None, 160)
    _one(pool, xa, None, 160, (640, 0.0))                                  # leaves the slot at gain 1
    again = _one(pool, xb, None, 160)                                      # the same slot: opens at 20 dB, no ramp
    assert torch.equal(again, fresh)
    _check_blend(again, xb, _one(_pool("c4", 1), xb, None, 160), AR.gain(20.0), "the slot's next session")
    _one(pool, xa, 3.0, None, (5 * HOP, 1.0))
    assert torch.equal(_one(pool, xb, None), fresh)


# ---------------------------------------------------------------- 11. the pool at 48 kHz
def _join_bound(up_y, up_x, x, G):
    """three roundings of the sum and three of the interpolation"""
    return 4 * U32 * np.abs(up_y) + 8 * U32 * G * (np.abs(x) + np.abs(up_x))


@pytest.mark.parametrize("mode", ["drop", "keep", "follow"])
def test_pool_at_48_khz_is_the_composition_with_the_limit_at_16_khz(mode):
    """As test_pool_at_another_rate_is_the_exact_composition: the session against resample down -> the 16 kHz pool WITH the
    limit -> resample up ("drop") or highband.rejoin ("keep"), bit for bit.  The causal "follow" has no offline composition
    to be equal to; it is held, as test_follow_join_matches_float64 holds it, to the float64 join of the same pieces within
    the bound of section 3r, with the limited 16 kHz signal in the place of ys16 -- in the gains too."""
    from tinyrecurrentunet_amd import highband as HB, resample as R, stream_highband as SH
    fs, lims = 48000, [6.0, 20.0, 0.0]
    pd, qd = R.ratio(fs, 16000)
    xs = _audio([769, 8195, 12007], seed=37)
    pool = _pool("c4", 4, fs=fs, highband=mode, atten_lim_db=12.0)
    ids = pool.open(4)[1:]
    pool.set_atten_lim(ids, lims)
    got = {s: [] for s in ids}
    at = dict.fromkeys(ids, 0)
    cuts = dict(zip(ids, (960, 441, 5000)))
    while at:
        live = list(at)
        outs = pool.feed([xs[ids.index(s)][at[s]:at[s] + cuts[s]] for s in live], live)
        for s, o in zip(live, outs):
            got[s].append(o)
            at[s] += cuts[s]
        done = [s for s in live if at[s] >= xs[ids.index(s)].shape[0]]
        for s, o in zip(done, pool.close(done) if done else []):
            got[s].append(o)
            del at[s]
    plain = _pool("c4", 1, atten_lim_db=12.0)
    for s, x, L in zip(ids, xs, lims):
        y = torch.cat(got[s])
        lo = R.resample([x], fs, 16000)[0]
        ys16 = _one(plain, lo, L, 1000)
        assert y.shape == x.shape and ys16.shape == lo.shape
        if mode == "drop":
            want = R.resample([ys16], 16000, fs)[0][:x.shape[0]]
        elif mode == "keep":
            want = HB.rejoin([x], [lo], [ys16], fs, "keep")[0]
        else:
            n = x.shape[0]
            up_y, up_x = R.resampler(16000, fs, "cuda")([ys16], x2=[lo])
            g = SH.block_gains([lo], [ys16])[0]
            x64, uy, ux = _np(x), _np(up_y[0])[:n], _np(up_x[0])[:n]
            G = SR.sample_gains(_np(g), n, pd, qd)
            err = np.abs(_np(y) - HR.join(uy, ux, x64, G))
            bound = _join_bound(uy, ux, x64, G)
            assert np.all(err <= bound), (n, float(np.max(err / np.maximum(bound, 1e-300))))
            continue
        assert torch.equal(y, want), (mode, x.shape[0], float((y - want).abs().max()))


# ---------------------------------------------------------------- 12. records and tables that leave the extents
def test_records_that_leave_the_extents_are_skipped():
    """Every buffer is larger than the extents the entry point is told, and filled with a canary: a record whose slot,
    packet, outputs or remainder lie outside the declared extents makes no store at all -- its workgroup returns -- and the
    good records beside it are carried out."""
    from tinyrecurrentunet_amd import _lib as L, atten as AT
    from tinyrecurrentunet_amd._lib import ptr
    lib, st = L.lib(), L.stream()
    CAN, S, S_REAL, NP, NO = 7.5, 8, 16, 512, 1024
    can = lambda *s: torch.full(s, CAN, device="cuda", dtype=torch.float32)
    g = torch.Generator(device="cuda").manual_seed(5)
    F, C = AT.FIRST, AT.CLOSING
    # slot, c0, poff, n, ooff, m, flags, 0
    recs = [[3, 384, 0, 128, 0, 128, 0, 0],            # good: a steady hop, ramping
            [8, 384, 128, 128, 128, 128, 0, 0],        # the slot is outside [0, 8)
            [-1, 384, 128, 128, 128, 128, 0, 0],
            [1, 384, 448, 128, 128, 128, 0, 0],        # the packet leaves the 512 samples declared
            [1, 384, -4, 128, 128, 128, 0, 0],
            [1, 384, 128, 128, 960, 128, 0, 0],        # the outputs leave the 1024 declared
            [1, 384, 128, 128, -128, 128, 0, 0],
            [1, 512, 128, 0, 128, 128, 0, 0],          # more in the line than it holds
            [1, 384, 128, 128, 128, 0, 0, 0],          # 512 would stay
            [1, 100, 128, 28, 128, 129, 0, 0],         # gives more than it has
            [1, 384, 128, 1, 128, 384, C, 0],          # a closing session that leaves a sample
            [1, 384, 128, 128, 128, 128, 4, 0],        # an unknown flag
            [1, 384, 128, -1, 128, 128, 0, 0],
            [5, 200, 256, 100, 256, 300, F | C, 0]]    # good: a short session closes, from its target
    tab = torch.tensor(recs, dtype=torch.int32, device="cuda")
    out, dry, g_cur, packet = can(2 * NO), can(S_REAL, AT.DRY_LINE), can(S_REAL), can(2 * NP)
    wet = torch.randn(NO, device="cuda", generator=g) * 0.1
    out[:NO] = wet
    dry[:S] = torch.randn((S, AT.DRY_LINE), device="cuda", generator=g) * 0.1
    packet[:NP] = torch.randn(NP, device="cuda", generator=g) * 0.1
    g_cur[:S] = 0.25
    g_tgt = torch.full((S_REAL,), 0.75, device="cuda")
    dry0, out0 = dry.clone(), out.clone()
    assert lib.trunet_stream_atten(ptr(out), ptr(dry), ptr(g_cur), ptr(g_tgt), ptr(packet), tab.data_ptr(), len(recs), S, NP,
                                   NO, st) == 0
    torch.cuda.synchronize()
    # the two good records
    line3 = torch.cat([dry0[3, :384], packet[:128]])
    _check_blend(out[:128], line3[:128], wet[:128], AR.ramp(0.25, 0.75), "record 0", np.ones(128, dtype=bool))
    assert torch.equal(dry[3, :384], line3[128:]) and float(g_cur[3]) == 0.75
    line5 = torch.cat([dry0[5, :200], packet[256:356]])
    _check_blend(out[256:556], line5, wet[256:556], 0.75, "record 13")
    assert torch.equal(dry[5], dry0[5]) and float(g_cur[5]) == 0.25        # a closing slot keeps nothing and writes nothing
    # everything else is as it was
    keep = torch.ones(2 * NO, dtype=torch.bool, device="cuda")
    keep[:128] = False
    keep[256:556] = False
    assert torch.equal(out[keep], out0[keep])
    rows = [r for r in range(S_REAL) if r != 3]
    assert torch.equal(dry[rows], dry0[rows]) and torch.equal(dry[3, 384:], dry0[3, 384:])
    assert torch.equal(g_cur[[0, 1, 2, 4, 6, 7]], torch.full((6,), 0.25, device="cuda")) and bool((g_cur[S:] == CAN).all())
    assert bool((packet[NP:] == CAN).all()) and bool((g_tgt == 0.75).all())

    # the ragged blend: utterances whose offsets contradict each other are left alone, and nothing is stored past the total
    total = 3000
    audio, x = can(2 * total), torch.randn(total, device="cuda", generator=g) * 0.1
    y = torch.randn(total, device="cuda", generator=g) * 0.1
    audio[:total] = y
    gains = torch.tensor([0.5, 0.25, 0.125, 1.0], device="cuda")
    off = torch.tensor([0, 1000, 600, 2000, 3500], dtype=torch.int64, device="cuda")     # 1 runs backwards, 3 leaves the total
    assert lib.trunet_atten_blend_ragged(ptr(audio), ptr(x), ptr(gains), off.data_ptr(), 4, total, st) == 0
    torch.cuda.synchronize()
    assert bool((audio[total:] == CAN).all())
    assert torch.equal(audio[2000:total], y[2000:])                        # utterance 3 claims samples past the total
    _check_blend(audio[1000:2000], x[1000:2000], y[1000:2000], 0.125, "utterance 2 of a corrupt table")
    # whichever utterance a sample below 1000 fell to, it is one of the blends or y itself
    cands = np.stack([AR.blend(_np(x[:1000]), _np(y[:1000]), gg) for gg in (0.5, 0.25, 0.125)] + [_np(y[:1000])])
    assert np.all(np.min(np.abs(cands - _np(audio[:1000])), axis=0) <= AR.bound(_np(x[:1000]), _np(y[:1000])))


# ---------------------------------------------------------------- 13. AudioStream
@pytest.mark.parametrize("cin,tgru", [(4, False), (3, False), (4, True)])
def test_audio_stream_with_limits(cin, tgru):
    from tinyrecurrentunet_amd.streaming import AudioStream
    net, S, hops = _net(cin, tgru), 4, 9
    x = torch.stack(_audio([HOP * hops] * S, seed=41))
    lims = [6.0, INF, 0.0, 20.0]

    def run(**kw):
        st = AudioStream(net, S, tgru=tgru, **kw)
        outs = [st.push(x[:, HOP * a:HOP * (a + 1)].contiguous()) for a in range(hops)]
        return torch.cat(outs + [st.flush()], 1)

    wet, out = run(), run(atten_lim_db=lims)
    assert out.shape == x.shape == wet.shape
    for s, L in enumerate(lims):
        _check_blend(out[s], x[s], wet[s], AR.gain(L), "AudioStream C_in %d stream %d at %g dB" % (cin, s, L))
    assert torch.equal(out[1], wet[1]) and not torch.equal(out[0], wet[0])
    assert torch.equal(run(atten_lim_db=INF), wet) and torch.equal(run(atten_lim_db=None), wet)
    assert torch.equal(run(atten_lim_db=20.0)[3], out[3])                  # a scalar is that limit for every stream
