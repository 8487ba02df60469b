"""Float64 numpy restatement of the stateful resampler (resample.py: StreamResampler), on top of
resample_ref's definition.

A test helper, independent of the package.  A stream that has received N samples of a session has emitted

    ready(N) = max(0, ceil((N p - half) / q))

outputs, keeps the session's last K - 1 samples, and computes every output from the line [history | packet] alone; ``close``
computes the outputs up to ceil(N p / q) with zeros to the right.  ``Stream.lowest`` records, per call, the lowest sample any
output of the call read, counted back from the samples received before the call (at most the history length, or the
history does not suffice).
"""
import numpy as np

import resample_ref as RR


def ready(N, p, q, half):
    return max(0, -((half - N * p) // q))


def history(p, half):
    return RR.taps_per_output(p, half) - 1


class Stream:
    def __init__(self, p, q, h=None):
        self.p, self.q = p, q
        if h is None:
            self.h, self.half = RR.design(p, q)
        else:
            self.h, self.half = np.asarray(h, dtype=np.float64), (len(h) - 1) // 2
        self.K = RR.taps_per_output(p, self.half)
        self.H = self.K - 1
        self.hist = np.zeros(self.H)
        self.N = self.E = 0
        self.lowest = []

    def _outputs(self, line, N0, N1, m0, m1):
        """outputs m0 .. m1 - 1 from the line, whose element i is sample N0 - H + i; samples outside [0, N1) are zero"""
        p, q, half = self.p, self.q, self.half
        if m1 <= m0:
            return np.zeros(0)
        m = np.arange(m0, m1, dtype=np.int64)
        k = np.arange(self.K)[None, :]
        nmax = (m * q + half) // p
        t = (m * q + half - nmax * p)[:, None] + p * k
        n = nmax[:, None] - k
        ok = (t <= 2 * half) & (n >= 0) & (n < N1)
        i = n - (N0 - self.H)
        if ok.any():
            self.lowest.append(int(N0 - n[ok].min()))
        assert not (ok & (i < 0)).any(), "an output reads a sample the history no longer holds"
        pad = np.concatenate([line, [0.0]])
        prod = np.where(ok, self.h[np.minimum(t, 2 * half)] * pad[np.where(ok, i, line.shape[0])], 0.0)
        return p * np.sum(prod, axis=1)

    def feed(self, x, closing=False):
        x = np.asarray(x, dtype=np.float64)
        N0, N1 = self.N, self.N + x.shape[0]
        line = np.concatenate([self.hist, x])
        target = -(-N1 * self.p // self.q) if closing else ready(N1, self.p, self.q, self.half)
        y = self._outputs(line, N0, N1, self.E, target)
        if closing:
            self.hist, self.N, self.E = np.zeros(self.H), 0, 0
        else:
            self.hist, self.N, self.E = line[line.shape[0] - self.H:], N1, target
        return y

    def close(self):
        return self.feed(np.zeros(0), closing=True)


def run(x, cuts, p, q, h=None):
    """x cut at the indices ``cuts`` (ascending, repeats = empty packets) through a fresh stream -> (list of feed results,
    close result, the stream)"""
    s = Stream(p, q, h)
    edges = [0] + [int(c) for c in cuts] + [len(x)]
    feeds = [s.feed(x[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    return feeds, s.close(), s
