"""The attenuation limit: "suppress by at most L dB", one definition for every inference route.

``atten_lim_db = None`` leaves a route exactly as it is.  ``atten_lim_db = L`` (a finite number >= 0, or ``inf``) sets
g = 10^(-L / 20), computed in float64 and rounded to fp32, and the route returns

    out[n] = y[n] + g (x[n] - y[n])

with y the 16 kHz sample it returns without a limit and x the dry 16 kHz input sample at the same position: fp32, one
subtraction and one fused multiply-add (csrc/atten_blend.hpp).  L = 0 returns the input, L = inf (g = 0) the unlimited
result bit for bit.  The blend acts at 16 kHz directly behind the overlap-add; what follows -- resampling back to ``fs``,
``highband="keep"``, the ``"follow"`` gain -- reads the blended signal.

In the stream pool a session's limit may move while it runs (``StreamPool.set_atten_lim``): over the 128 samples of the
first hop the session emits after the call the gain goes from the old value to the new one,
g_i = g_old + (g_new - g_old) (i + 1) / 128, and is g_new from then on.

Host side only: validation, L -> g, and the per-call plan of the pool's launch (``plan_atten``); the launches live with
their routes (enhance.py, streaming.py) on csrc/atten.hip.
"""
import math
import numbers

import numpy as np
import torch

HOP = 128
INTS = 8                     # trunet_hip.h: TRUNET_ATT_INTS
DRY_LINE = 512               # TRUNET_ATT_DRY_LINE: floats of a slot's dry line
DRY_BOUND = 4 * HOP - 1      # a hop comes back four hops after it arrived: 128 min(a, 3) + pending <= 511 samples wait
FIRST, CLOSING = 1, 2        # TRUNET_ATT_FIRST, TRUNET_ATT_CLOSING


def gain(atten_lim_db):
    """L in dB -> g = 10^(-L / 20) as np.float32; 0 -> 1, inf -> 0.  ValueError for anything but a finite number >= 0 or
    inf: negative values, NaN, bool, other types."""
    v = atten_lim_db
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (numbers.Real, np.integer, np.floating)):
        raise ValueError("atten_lim_db: a number of dB >= 0 or inf, got %r" % (v,))
    v = float(v)
    if math.isnan(v) or v < 0.0:
        raise ValueError("atten_lim_db: a number of dB >= 0 or inf, got %r" % (atten_lim_db,))
    return np.float32(0.0 if math.isinf(v) else 10.0 ** (-v / 20.0))


def gains(atten_lim_db, n, what="utterances"):
    """A scalar, or one value per entry as a sequence or 1-D tensor of length n -> (n,) np.float32 gains.  ValueError as
    ``gain``, and for a sequence of another length."""
    v = atten_lim_db
    if torch.is_tensor(v):
        if v.dtype == torch.bool:
            raise ValueError("atten_lim_db: numbers of dB, got a bool tensor")
        v = v.detach().cpu().tolist()
    elif isinstance(v, np.ndarray):
        if v.dtype == np.bool_:
            raise ValueError("atten_lim_db: numbers of dB, got a bool array")
        v = v.tolist()
    if isinstance(v, (list, tuple)):
        if len(v) != n:
            raise ValueError("atten_lim_db: %d values for %d %s" % (len(v), n, what))
        return np.array([gain(e) for e in v], dtype=np.float32)
    return np.full(n, gain(v), dtype=np.float32)


def plan_atten(slots, dry_count, packet_off, packet_lens, out_off, out_lens, first, closing):
    """The records of one trunet_stream_atten launch, host only.  Per listed session: its slot, the samples in its dry line
    before the call, where its new samples lie in the call's packet buffer and how many they are, where its outputs lie in
    the call's output and how many they are, whether the call holds its frame 0.  closing: the call ends every listed
    session.  -> ((n, INTS) int32 table, samples in each dry line after the call).  AssertionError where a line would
    give more than it holds or keep more than ``DRY_BOUND``: the pool's own counters never get there."""
    cols = [np.asarray(v, dtype=np.int64).reshape(-1) for v in (slots, dry_count, packet_off, packet_lens, out_off, out_lens)]
    slot, c0, poff, n, ooff, m = cols
    k = slot.shape[0]
    if any(c.shape[0] != k for c in cols):
        raise ValueError("plan_atten: %s entries for %d sessions" % ([c.shape[0] for c in cols], k))
    keep = c0 + n - m
    poff, ooff = np.where(n > 0, poff, 0), np.where(m > 0, ooff, 0)      # an empty span lies at 0: inside any extent
    if (keep < 0).any() or (closing and keep.any()) or (not closing and k and int(keep.max()) > DRY_BOUND):
        raise AssertionError("attenuation limit: a dry line would hold %s samples (a bound of DESIGN section 3s does not hold)"
                             % keep.tolist())
    table = np.zeros((k, INTS), dtype=np.int32)
    flags = np.where(np.asarray(first, dtype=bool).reshape(-1), FIRST, 0) | (CLOSING if closing else 0)
    for c, v in enumerate((slot, c0, poff, n, ooff, m, flags)):
        table[:, c] = v
    return table, keep
