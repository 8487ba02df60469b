"""The band above 8 kHz for the stream pool at fs > 16 kHz: ``highband``'s "keep" and a causal "follow"
for sessions that arrive in packets, without added latency.

For one session x of L samples at ``fs``, with (pd, qd) = ratio(fs, 16000), lo = D(x) (L16 samples), ys16 what the 16 kHz
pool returns for lo, up_y = U(ys16)[:L], up_x = U(lo)[:L]:

    "keep":    out = up_y + (x - up_x)                      bit for bit ``highband.rejoin([x], [lo], [ys16], fs, "keep")[0]``
    "follow":  out[n] = fmaf(G[n], x[n] - up_x[n], up_y[n]) with a gain every sample can know when it is emitted:
        hp = highband.highpass();  a[n] = sum_{k = 0 .. 62} hp[k] lo[n - k], b the same on ys16   (3p's filter, 31 samples late)
        E_x[j], E_y[j] = sum of a^2, b^2 over hop block j = [128 j, 128 j + 128) n [0, L16),  j < J = ceil(L16 / 128)
        g_c[j] = clamp(sqrt((sum_{i = max(j - 3, 0) .. j} E_y[i] + 1e-10) / (sum_i E_x[i] + 1e-10)), 10^(floor_db / 20), 1)
        s = n pd, D = 128 qd, j = s // D, c = s % D:   G[n] = ((D - c) g_c[max(j - 1, 0)] + c g_c[j]) / D

The gain trails the suppression it follows by about two hops plus the filter's 2 ms: a definition, not a defect; it is not
offline "follow" (which looks two hops ahead).  Per slot the pool keeps (``StreamHighband``): the x line, the samples at
``fs`` fed and not yet returned, at most ``x_line_bound(pd, qd)``; the lo line, the samples of lo whose ys16 has not come
back, at most 511; a third ``StreamResampler`` plane 16 kHz -> fs for lo, which shares the up-resampler's plan; and for
"follow" the last 62 samples of lo and ys16, the last three block energies and the last two block gains.  A call is one
int64 plan (``plan_highband``), made before the first launch, and trunet_stream_highband_pair, the lo plane,
trunet_stream_highband_gains ("follow"), trunet_stream_highband_join and trunet_stream_highband_commit
(stream_highband.hip); nothing is read back.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from . import highband as HB
from ._lib import check, ptr

SAMPLE_RATE, HOP = HB.SAMPLE_RATE, HB.HOP
HALO = HB.TAPS - 1           # samples of lo and ys16 a slot keeps left of the next block
INTS = 18                    # trunet_hip.h: TRUNET_SHB_INTS
LO_LINE = 512                # TRUNET_SHB_LO_LINE: floats of a slot's lo line
MAX_X_LINE = 4096            # TRUNET_SHB_MAX_X_LINE: floats of a slot's x line, at most
TILE = 1024                  # TRUNET_SHB_TILE
LO_BOUND = 4 * HOP - 1       # the 16 kHz pool returns hop a - 4 with hop a: 128 min(a, 3) + pending <= 511 samples wait
LOOKAHEAD = 16               # resample.ZEROS: samples at 16 kHz either resampler waits for
INT32_MAX = 2 ** 31 - 1

# table: (n, INTS) int64, the records the kernels read (trunet_hip.h); x_count, lo_count, blocks: per listed session AFTER
# the call (0 for a closing one); out_off, out_lengths: where each session's samples lie in the call's output
HbPlan = namedtuple("HbPlan", "table x_count lo_count blocks out_off out_lengths n_packet n_up n_x16 n_paired n_blocks "
                              "n_join_tiles n_pair_tiles closing moves")


def x_line_bound(pd, qd):
    """The most samples at fs a session has been fed and not been given back, after any call.  With F samples fed, the
    down-resampler has delivered n16 = ready(F) >= F pd / qd - 16 samples of lo, the 16 kHz pool has returned
    Y = 128 max(n16 // 128 - 3, 0) >= n16 - 511 of them, and the up-resampler has emitted E = ready(Y) >= (Y - 16) qd / pd,
    so F - E <= (511 + 2 * 16) qd / pd, an integer."""
    return (LO_BOUND + 2 * LOOKAHEAD) * qd // pd


def _broken(what):
    raise AssertionError("stream highband: %s (a bound of DESIGN section 3r does not hold)" % what)


def plan_highband(slots, x_count, lo_count, blocks, emitted, packet_lens, x16_lens, pair_lens, up_off, out_lens, n_up,
                  closing, xcap):
    """What one call owes, host only.  Per listed session: its slot; samples in its x and lo lines, hop blocks complete and
    outputs emitted BEFORE the call; samples in its packet, of lo that packet produced (x16) and of ys16 the 16 kHz pool
    returns in this call; where its outputs start in the up-resamplers' packed outputs (n_up in all) and how many of them
    are written.  closing: the call ends every listed session.  AssertionError, with nothing changed, where an occupancy
    would pass its bound."""
    cols = [np.asarray(v, dtype=np.int64).reshape(-1) for v in (slots, x_count, packet_lens, up_off, out_lens, lo_count,
                                                                x16_lens, pair_lens, emitted, blocks)]
    slot, xc0, xn, uoff, on, lc0, ln, pn, e0, b0 = cols
    n = slot.shape[0]
    if any(c.shape[0] != n for c in cols):
        raise ValueError("plan_highband: %s entries for %d sessions" % ([c.shape[0] for c in cols], n))
    closing = bool(closing)
    xc1, lc1 = xc0 + xn - on, lc0 + ln - pn
    if (on < 0).any() or (pn < 0).any() or (xc1 < 0).any() or (lc1 < 0).any():
        _broken("a line gives more than it holds: x %s, lo %s" % (xc1.tolist(), lc1.tolist()))
    if closing:
        if xc1.any() or lc1.any():
            _broken("a closing session leaves samples behind: x %s, lo %s" % (xc1.tolist(), lc1.tolist()))
        bn = -(-pn // HOP)
    else:
        if (pn % HOP).any():
            _broken("an open session got ys16 that is not whole hops: %s" % pn.tolist())
        if n and (int(xc1.max()) > xcap or int(lc1.max()) > LO_BOUND):
            _broken("x line %d of %d, lo line %d of %d" % (int(xc1.max()), xcap, int(lc1.max()), LO_BOUND))
        bn = pn // HOP
    n_packet, n_x16, n_paired, n_blocks = (int(v.sum()) for v in (xn, ln, pn, bn))
    if max(n_packet, n_x16, n_paired, int(n_up)) > INT32_MAX:
        raise ValueError("%d samples in one call: a call packs fewer than 2^31" % max(n_packet, n_x16, n_paired, int(n_up)))
    jt, pt = -(-on // TILE), -(-pn // TILE)
    table = np.zeros((n, INTS), dtype=np.int64)
    for c, v in enumerate((slot, xc0, np.cumsum(xn) - xn, xn, uoff, on, lc0, np.cumsum(ln) - ln, ln, np.cumsum(pn) - pn, pn,
                           e0, b0, bn, np.cumsum(jt) - jt, closing, np.cumsum(pt) - pt, np.cumsum(bn) - bn)):
        table[:, c] = v
    zero = np.zeros(n, dtype=np.int64)
    moves = not closing and bool(((xn > 0) | (on > 0) | (ln > 0) | (pn > 0)).any())
    return HbPlan(table, zero if closing else xc1, zero if closing else lc1, zero if closing else b0 + bn, uoff.tolist(),
                  on.tolist(), n_packet, int(n_up), n_x16, n_paired, n_blocks, int(jt.sum()), int(pt.sum()), closing, moves)


class _State:
    """the per-slot device buffers of ``slots`` sessions (trunet_hip.h)"""

    def __init__(self, slots, xcap, follow, dev):
        z = lambda *s: torch.zeros(s, device=dev, dtype=torch.float32)
        self.x_line, self.lo_line = z(slots, xcap), z(slots, LO_LINE)
        self.halo, self.energy, self.gain = (z(slots, HALO, 2), z(slots, 3, 2), z(slots, 2)) if follow else (None,) * 3


def _gains(lib, st, state, plan, ext, tab, paired, ys16, floor_db, dev):
    """the "follow" launches of a call -> (eline, gline)"""
    n = len(plan.table)
    eline = torch.empty((plan.n_blocks + 3 * n, 2), device=dev, dtype=torch.float32)
    gline = torch.empty(plan.n_blocks + 2 * n, device=dev, dtype=torch.float32)
    check(lib.trunet_stream_highband_gains(ptr(paired), ptr(ys16), ptr(state.halo), ptr(state.energy), ptr(state.gain),
                                           ptr(HB._taps(dev)), ptr(eline), ptr(gline), tab.data_ptr(), *ext,
                                           HB.floor_gain(floor_db), st), "stream_highband_gains")
    return eline, gline


class StreamHighband:
    """The per-slot state and the launches that carry the band above 8 kHz around a ``StreamPool`` at ``fs`` > 16 kHz
    (module docstring).  Host counters per slot: samples in the x line, samples in the lo line, hop blocks complete.  The
    device buffers come with the first call that reaches the device.  ValueError at construction for a rate whose x line
    would exceed ``MAX_X_LINE`` floats."""

    def __init__(self, fs, slots, mode, floor_db, device):
        from . import resample as R
        self.mode, self.floor_db = HB.check_args(mode, floor_db)
        self.fs, self.slots, self.device = int(fs), int(slots), torch.device(device)
        self.pd, self.qd = R.ratio(fs, SAMPLE_RATE)
        if self.mode == "drop" or self.pd >= self.qd:
            raise ValueError("a StreamHighband is for \"keep\" and \"follow\" above %d Hz" % SAMPLE_RATE)
        self.xcap = x_line_bound(self.pd, self.qd)
        if self.xcap > MAX_X_LINE:
            raise ValueError("%d Hz would keep up to %d samples per session, and a slot's line holds at most %d"
                             % (self.fs, self.xcap, MAX_X_LINE))
        self.up_lo = R.StreamResampler(SAMPLE_RATE, self.fs, self.slots, self.device)      # the third plane: U(lo)
        self._xc = np.zeros(self.slots, dtype=np.int64)
        self._lc = np.zeros(self.slots, dtype=np.int64)
        self._blk = np.zeros(self.slots, dtype=np.int64)
        self._state = None

    @property
    def state(self):
        if self._state is None:
            self._state = _State(self.slots, self.xcap, self.mode == "follow", self.device)
        return self._state

    def reset(self, ids):
        """the listed slots start afresh; host work only: a slot whose counts are zero reads nothing of its buffers"""
        self._xc[ids] = 0
        self._lc[ids] = 0
        self._blk[ids] = 0
        self.up_lo.reset(ids)

    def plan(self, ids, packet_lens, x16_lens, pair_lens, pu, emitted, out_lens=None, closing=False):
        """the plan of a call; pu: the up-resampler's plan of the call, emitted: its counts before the call"""
        return plan_highband(ids, self._xc[ids], self._lc[ids], self._blk[ids], emitted, packet_lens, x16_lens, pair_lens,
                             pu.out_off, pu.lengths if out_lens is None else out_lens, pu.n_out, closing, self.xcap)

    def run(self, plan, pu, packet, x16, ys16, up_y, ids):
        """Carry out ``plan``: packet, x16, ys16: the call's packets at fs, their lo, and the 16 kHz pool's result, each back
        to back (None when empty); up_y: the up-resampler's outputs of the call -> the call's output, packed like up_y."""
        dev, lib, st, s = self.device, L.lib(), L.stream(), self.state
        mode = HB.FOLLOW if self.mode == "follow" else HB.KEEP
        ext = (len(plan.table), self.slots, self.xcap, plan.n_packet, plan.n_up, plan.n_x16, plan.n_paired, plan.n_blocks)
        tab = torch.from_numpy(plan.table).to(dev)                          # ONE copy
        paired = torch.empty(plan.n_paired, device=dev, dtype=torch.float32) if plan.n_paired else None
        if plan.n_paired:
            check(lib.trunet_stream_highband_pair(ptr(s.lo_line), ptr(x16), ptr(paired), tab.data_ptr(), *ext,
                                                  plan.n_pair_tiles, st), "stream_highband_pair")
        up_x = self.up_lo.run(pu, paired, ids)
        eline = gline = None
        if mode == HB.FOLLOW:
            eline, gline = _gains(lib, st, s, plan, ext, tab, paired, ys16, self.floor_db, dev)
        out = torch.empty(plan.n_up, device=dev, dtype=torch.float32)
        if plan.n_join_tiles:
            check(lib.trunet_stream_highband_join(ptr(up_y), ptr(up_x), ptr(s.x_line), ptr(packet), ptr(gline), ptr(out),
                                                  tab.data_ptr(), *ext, plan.n_join_tiles, self.pd, self.qd, mode, st),
                  "stream_highband_join")
        if plan.moves:
            check(lib.trunet_stream_highband_commit(ptr(s.x_line), ptr(packet), ptr(s.lo_line), ptr(x16), ptr(s.halo),
                                                    ptr(paired), ptr(ys16), ptr(s.energy), ptr(eline), ptr(s.gain),
                                                    ptr(gline), tab.data_ptr(), *ext, mode, st), "stream_highband_commit")
        self._xc[ids], self._lc[ids], self._blk[ids] = plan.x_count, plan.lo_count, plan.blocks
        return out


@torch.no_grad()
def block_gains(lo, ys16, floor_db=HB.FLOOR_DB):
    """lo, ys16: lists of 1-D cuda tensors at 16 kHz, session by session of equal lengths -> the list of their causal block
    gains g_c (ceil(L16 / 128) each), from trunet_stream_highband_gains with every session whole in one closing record.
    Block sums have one order however a session is cut, so these are the gains a pool computes for it."""
    _, floor_db = HB.check_args("follow", floor_db)
    dev, lens = HB._signals("lo", lo)
    _, lens_y = HB._signals("ys16", ys16, dev)
    if lens_y != lens:
        raise ValueError("ys16 must have the lengths of lo: %s against %s" % (lens_y, lens))
    if not lens:
        return []
    n, zero = len(lens), np.zeros(len(lens), dtype=np.int64)
    plan = plan_highband(np.arange(n), zero, zero, zero, zero, zero, lens, lens, zero, zero, 0, True, 1)
    ext = (n, n, 1, 0, 0, plan.n_x16, plan.n_paired, plan.n_blocks)
    tab = torch.from_numpy(plan.table).to(dev)
    _, gline = _gains(L.lib(), L.stream(), _State(n, 1, True, dev), plan, ext, tab, HB._cat(lo), HB._cat(ys16), floor_db, dev)
    blocks = plan.table[:, 13].tolist()
    return [gline[o + 2 * i + 2:o + 2 * i + 2 + b] for i, (o, b) in enumerate(zip(plan.table[:, 17].tolist(), blocks))]
