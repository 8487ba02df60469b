"""No GPU: the host side of StreamPool.feed (tinyrecurrentunet_amd/streaming.py: plan_feed) against a loop over plan_step,
and the argument checks of the four trunet_stream_feed_* entry points."""
import subprocess
import sys

import numpy as np
import pytest

HOP = 128
A0S = [0, 1, 2, 3, 4, 5, 6, 10 ** 6]
R0S = [0, 1, 64, 127]
NS = [0, 1, 127, 128, 129, 160, 320, 511, 1000]


def _sm():
    from tinyrecurrentunet_amd import streaming
    return streaming


def _by_steps(a0, a1):
    """(frame, FIRST / STASHED flags, env, emits) of every frame a single session owes when it goes from a0 to a1 whole hops
    through plan_step, one hop per step, in the order the passes run"""
    sm = _sm()
    rows, hops = [], np.array([a0], dtype=np.int64)
    for _ in range(a1 - a0):
        plan = sm.plan_step(hops, [0])
        for table, nf in zip(plan.tables, plan.frames):
            for r in sm.rows_of(table[:nf]):
                rows.append((r.frame, r.flags & (sm.ROW_FIRST | sm.ROW_STASHED), r.env, r.out >= 0))
        hops[0] = plan.hops[0]
    assert hops[0] == a1
    return rows


def _by_feed(plan, k=0):
    """the same of session k (position in the call) of a feed plan, in frame order, and the hops of `out` it fills"""
    sm = _sm()
    rec = sm.feed_rows_of(plan.rows)
    (s,) = [v for v in plan.sess if v[9] == k]
    mine = [rec[i] for i in plan.seq[s[2]:s[2] + s[3]]]
    return ([(r.frame, r.flags & (sm.ROW_FIRST | sm.ROW_STASHED), r.env, r.out >= 0) for r in mine],
            [r.out for r in mine if r.out >= 0])


def test_plan_feed_needs_no_library():
    code = ("import tinyrecurrentunet_amd._lib as L\n"
            "L.LIB_PATH = '/nonexistent/libtrunet_hip.so'\n"
            "from tinyrecurrentunet_amd.streaming import plan_feed\n"
            "p = plan_feed([0, 5], [0, 7], [1000, 160], [1, 0])\n"
            "assert L._lib is None\n"
            "print(len(p.rows), p.lengths)\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[0] == "7"            # slot 1: hops 5 -> 12, frames 4..10; slot 0 only stores


@pytest.mark.parametrize("a0", A0S)
def test_plan_feed_matches_a_loop_over_plan_step(a0):
    sm = _sm()
    for r0 in R0S:
        for n in NS:
            a1, r1 = (HOP * a0 + r0 + n) // HOP, (r0 + n) % HOP
            plan = sm.plan_feed([a0], [r0], [n], [0])
            got, outs = _by_feed(plan)
            assert got == _by_steps(a0, a1), (a0, r0, n)
            # contract item 2
            frames = [g[0] for g in got]
            want = ([0, 1] if a1 >= 3 > a0 else []) + list(range(max(a0 - 1, 2), a1 - 2 + 1))
            assert frames == want, (a0, r0, n)
            assert plan.hops.tolist() == [a1] and plan.pending.tolist() == [r1]
            assert plan.lengths == [HOP * (max(a1 - 3, 0) - max(a0 - 3, 0))]
            assert outs == list(range(len(outs))) and HOP * len(outs) == plan.lengths[0] == HOP * plan.n_out
            assert plan.n_samples == n and plan.n_active == (1 if frames else 0)
            # frames 0 and 1 are one transform: FIRST names the STASHED record
            rec = sm.feed_rows_of(plan.rows)
            for i, r in enumerate(rec):
                assert r.slot == 0 and (r.r0, r.n, r.poff) == (r0, n, 0)
                if r.flags & sm.ROW_FIRST:
                    assert r.frame == 0 and rec[r.pair].frame == 1 and rec[r.pair].flags & sm.ROW_STASHED and r.pair != i
                    assert r.off == 512 - HOP * a0 and r.off + 384 <= 512 + r0 + n
                elif not r.flags & sm.ROW_STASHED:
                    assert r.pair == -1 and r.off == HOP * (r.frame - a0) + 256 and 0 <= r.off <= r0 + n
            # depth d holds the d-th new frame
            assert plan.depths == [(d, d + 1) for d in range(len(frames))]
            assert plan.rows.dtype == plan.sess.dtype == plan.seq.dtype == np.int32


def test_several_sessions_side_by_side():
    sm = _sm()
    g = np.random.default_rng(5)
    for trial in range(40):
        S = int(g.integers(1, 12))
        cap = S + 3
        listed = g.permutation(cap)[:S]
        hops, pend = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
        hops[listed], pend[listed] = g.integers(0, 8, S), g.integers(0, HOP, S)
        n = g.integers(0, 1200, S) * (g.random(S) > 0.2)
        plan = sm.plan_feed(hops, pend, n, listed)
        rec = sm.feed_rows_of(plan.rows)
        assert sorted(plan.seq.tolist()) == list(range(len(rec)))                 # every frame row in exactly one list
        assert sorted(int(v[9]) for v in plan.sess) == list(range(S))
        outs = []
        for k in range(S):
            a0, r0 = int(hops[listed[k]]), int(pend[listed[k]])
            a1 = (HOP * a0 + r0 + int(n[k])) // HOP
            got, out = _by_feed(plan, k)
            assert got == _by_steps(a0, a1)
            assert out == list(range(int(plan.out_off[k]), int(plan.out_off[k]) + plan.lengths[k] // HOP))
            outs += out
            (s,) = [v for v in plan.sess if v[9] == k]
            assert s[0] == listed[k] and s[4] == a1 - a0 and (s[5], s[6]) == (r0, n[k]) and s[8] == (r0 + n[k]) % HOP
            assert s[7] == int(n[:k].sum())                                        # packets back to back
            assert all(rec[i].slot == listed[k] and rec[i].poff == s[7] for i in plan.seq[s[2]:s[2] + s[3]])
        assert sorted(outs) == list(range(plan.n_out))                             # output hops: disjoint, no gaps
        assert plan.hops.tolist() == [(HOP * hops[s] + pend[s] + m) // HOP for s, m in zip(listed, n)]
        # depth-major: slice d is the d-th new frame of the first hi - lo sessions, most frames first
        fr = plan.sess[:, 3]
        assert (np.diff(fr) <= 0).all() and plan.n_active == int((fr > 0).sum())
        at = 0
        for d, (lo, hi) in enumerate(plan.depths):
            assert lo == at and hi - lo == int((fr > d).sum())
            assert [plan.seq[plan.sess[j, 2] + d] for j in range(hi - lo)] == list(range(lo, hi))
            at = hi
        assert at == len(rec)


def test_packetisation_plans_the_same_frames():
    sm = _sm()
    g = np.random.default_rng(9)
    for total in (257, 384, 1000, 1407, 4000):
        want = None
        for cut in range(6):
            sizes, left = [], total
            while left:
                m = min(left, int(g.integers(0, [2, 130, 161, 400, 2000, 5000][cut])))
                sizes.append(m)
                left -= m
            hops, pend, seen, n_out = np.zeros(1, np.int64), np.zeros(1, np.int64), [], 0
            for m in sizes:
                plan = sm.plan_feed(hops, pend, [m], [0])
                seen += [(r.frame, r.env) for r in sm.feed_rows_of(plan.rows)]
                n_out += plan.lengths[0]
                hops[0], pend[0] = plan.hops[0], plan.pending[0]
            assert (hops[0], pend[0]) == (total // HOP, total % HOP)
            assert n_out == HOP * max(total // HOP - 3, 0)
            assert [f for f, _ in seen] == list(range(max(total // HOP - 1, 0))) if total >= 384 else seen == []
            want = sorted(seen) if want is None else want
            assert sorted(seen) == want


def test_misuse_is_refused_with_the_state_unchanged():
    sm = _sm()
    hops, pend = np.array([4, 0, 9], np.int64), np.array([5, 0, 100], np.int64)
    h0, p0 = hops.copy(), pend.copy()
    for lengths, listed in (([10, 10], [1, 1]),                  # a slot twice
                            ([10], [0, 1]), ([10, 10, 10], [0, 1]), ([[10, 10]], [0, 1]),       # lengths do not match the ids
                            ([10, -1], [0, 1]),                  # negative
                            ([1.5, 2.0], [0, 1]),
                            ([2 ** 31, 5], [0, 1]), ([2 ** 30, 2 ** 30], [0, 1]), ([2 ** 62, 2 ** 62], [0, 1])):   # beyond int32
        with pytest.raises(ValueError):
            sm.plan_feed(hops, pend, lengths, listed)
        assert (hops == h0).all() and (pend == p0).all()
    plan = sm.plan_feed(hops, pend, [], [])                      # an empty call is no misuse
    assert len(plan.rows) == len(plan.sess) == 0 and plan.lengths == [] and plan.depths == []


def test_feed_entry_points_reject_null_and_bad_counts():
    """The pattern of test_host_cpu.test_entry_points_reject_null_and_bad_shapes: TRUNET_EINVAL on the host, no launch."""
    from tinyrecurrentunet_amd import _lib
    lib, E = _lib.lib(), _lib.TRUNET_EINVAL
    P = [0x1000 * (i + 1) for i in range(9)]
    pc = (1e-6, 0.025, 0.98, 2.0, 0.5)

    def feats(ring=P[0], fifo=P[1], smp=P[2], feat=P[3], rows=P[4], n_rows=3, n_samples=100, slots=4, tw=P[5], C=4):
        return lib.trunet_stream_feed_features(ring, fifo, smp, feat, rows, n_rows, n_samples, slots, tw, C, None)

    for kw in (dict(ring=None), dict(fifo=None), dict(smp=None), dict(feat=None), dict(rows=None), dict(tw=None),
               dict(n_rows=0), dict(n_rows=-1), dict(n_samples=-1), dict(n_samples=0x7fff0001), dict(slots=0), dict(slots=-2),
               dict(C=2), dict(C=5)):
        assert feats(**kw) == E, kw

    def commit(ring=P[0], fifo=P[1], smp=P[2], M=P[3], feat=P[4], rows=P[5], sess=P[6], seq=P[7], n_sess=2, n_rows=3,
               n_samples=100, slots=4, C=4):
        return lib.trunet_stream_feed_commit(ring, fifo, smp, M, feat, rows, sess, seq, n_sess, n_rows, n_samples, slots, C,
                                             *pc, None)

    for kw in (dict(ring=None), dict(fifo=None), dict(smp=None), dict(M=None), dict(feat=None), dict(rows=None),
               dict(sess=None), dict(seq=None), dict(n_sess=0), dict(n_sess=-1), dict(n_rows=-1), dict(n_samples=-1),
               dict(n_samples=0x7fff0001), dict(slots=0), dict(C=0), dict(C=8)):
        assert commit(**kw) == E, kw

    def mask(y=P[0], frames=P[1], n_rows=3, tw=P[2]):
        return lib.trunet_stream_feed_mask_istft(y, frames, n_rows, tw, 0.5, None)

    for kw in (dict(y=None), dict(frames=None), dict(tw=None), dict(n_rows=0), dict(n_rows=-7)):
        assert mask(**kw) == E, kw

    def ola(frames=P[0], ol=P[1], out=P[2], rows=P[3], sess=P[4], seq=P[5], n_sess=2, n_rows=3, n_out=3, slots=4):
        return lib.trunet_stream_feed_ola(frames, ol, out, rows, sess, seq, n_sess, n_rows, n_out, slots, None)

    for kw in (dict(frames=None), dict(ol=None), dict(out=None), dict(rows=None), dict(sess=None), dict(seq=None),
               dict(n_sess=0), dict(n_sess=-1), dict(n_sess=4), dict(n_rows=0), dict(n_out=-1), dict(slots=0)):
        assert ola(**kw) == E, kw
