"""numpy restatement of the attenuation limit (tinyrecurrentunet_amd/atten.py, csrc/atten_blend.hpp), in
float64, for the tests: the gain of a limit, the blend, the ramp of a live change and the bounds both are held to.

    g = 10^(-L / 20), rounded to fp32            out[n] = y[n] + g (x[n] - y[n])
    a change from g_old to g_new:                g_i = g_old + (g_new - g_old) (i + 1) / 128 over the 128 samples of the
                                                 first hop the session emits after the call, g_new from then on

The blend is two or three fp32 roundings of quantities no larger than |x| + |y|, so an fp32 result lies within
4 * 2^-24 (|x| + |y|) of the float64 value; inside a ramp hop the fp32 rounding of g_i adds as much again: 8 * 2^-24."""
import math

import numpy as np

HOP = 128
U32 = 2.0 ** -24


def gain(atten_lim_db):
    """the fp32 gain of a limit in dB (inf -> 0), as a float64 number"""
    if math.isinf(atten_lim_db):
        return 0.0
    return float(np.float32(10.0 ** (-float(atten_lim_db) / 20.0)))


def blend(x, y, g):
    """y + g (x - y) in float64; g a number or one value per sample"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return y + np.asarray(g, dtype=np.float64) * (x - y)


def bound(x, y, roundings=4):
    return roundings * U32 * (np.abs(np.asarray(x, dtype=np.float64)) + np.abs(np.asarray(y, dtype=np.float64)))


def ramp(g_old, g_new):
    """the 128 gains of the hop over which a limit moves; the last one is g_new itself"""
    i = np.arange(HOP, dtype=np.float64)
    g = g_old + (g_new - g_old) * (i + 1.0) / HOP
    g[-1] = g_new
    return g


def session_gains(n, g_open, changes=()):
    """The gain of every output sample of a session of n samples (16 kHz) that opens with gain g_open, and whether the
    sample lies in a ramp hop.  changes: (P, g_new) in order, the limit moved when the session had been fed P samples.  By
    then it has emitted max(P // 128 - 3, 0) hops, so the ramp covers output hop h = max(P // 128 - 3, 0); a change before
    the session's frame 0 (P < 384: fewer than three hops) moves the gain the session starts with, without a ramp."""
    g = np.full(n, float(g_open), dtype=np.float64)
    in_ramp = np.zeros(n, dtype=bool)
    cur = float(g_open)
    for P, g_new in changes:
        if P < 3 * HOP:
            g[:] = g_new
        else:
            s = HOP * max(P // HOP - 3, 0)
            r = ramp(cur, g_new)[:max(min(HOP, n - s), 0)]
            g[s:s + len(r)] = r
            in_ramp[s:s + len(r)] = True
            g[s + len(r):] = g_new
        cur = float(g_new)
    return g, in_ramp


LINE, FIRST, CLOSING = 512, 1, 2


def stream_atten(table, out, dry_line, g_cur, g_tgt, packet, slots=None):
    """trunet_stream_atten restated (trunet_hip.h): per record, in place on out (n_out), dry_line (slots, 512) and g_cur
    (slots); packet (n_packet) and g_tgt (slots) are read.  A record that leaves the extents changes nothing.  float64
    arrays in, so what comes out is the value the fp32 kernel is held to.  -> the records that were carried out."""
    slots = dry_line.shape[0] if slots is None else slots
    done = []
    for i, (slot, c0, poff, n, ooff, m, flags, _) in enumerate(np.asarray(table).tolist()):
        keep = c0 + n - m
        ok = 0 <= slot < slots and not flags & ~(FIRST | CLOSING) and 0 <= c0 < LINE
        ok = ok and poff >= 0 and n >= 0 and poff + n <= packet.shape[0] and ooff >= 0 and m >= 0 and ooff + m <= out.shape[0]
        ok = ok and (keep == 0 if flags & CLOSING else 0 <= keep < LINE)
        if not ok:
            continue
        done.append(i)
        line = np.concatenate([dry_line[slot, :c0], packet[poff:poff + n]])
        tgt = g_tgt[slot]
        cur = tgt if flags & FIRST else g_cur[slot]
        g = np.full(m, tgt, dtype=np.float64)
        if cur != tgt:
            g[:HOP] = ramp(cur, tgt)[:min(m, HOP)]
        out[ooff:ooff + m] = blend(line[:m], out[ooff:ooff + m], g)
        if flags & CLOSING:
            continue
        dry_line[slot, :keep] = line[m:]
        if flags & FIRST or m > 0:
            g_cur[slot] = tgt
    return done
