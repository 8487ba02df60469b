#!/usr/bin/env python3
"""Golden values of the REFERENCE's own CosSimLoss (build container only).

Run from the repo root:  python tests/golden/make_cos_loss_golden.py
Imports /root/reference/cos_loss.py at run time (never copied) and evaluates its unmodified ``CosSimLoss()`` (default eps
and g = [508, 1016, 2032, 4062], cos_loss.py:23-25) on two B = 1 float32 pairs: L = 4224 (every segment whole) and
L = 2944 (shorter than g[-1] = 4062: the last segment is clipped by the slice).  B = 1 is the only batch size its forward
accepts (cos_loss.py:56).  Writes tests/golden/cos_loss.npz: x_<L>, y_<L> (1, L) and loss_<L> (the returned value).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def pair(length, seed):
    g = np.random.default_rng(seed)
    y = (0.1 * g.standard_normal((1, length)) + 0.01).astype(np.float32)
    x = (y + 0.03 * g.standard_normal((1, length))).astype(np.float32)
    return x, y


if __name__ == "__main__":
    sys.path.insert(0, REF)
    import cos_loss as ref_cos            # the reference's module
    assert ref_cos.__file__.startswith(REF)
    out = {}
    for length, seed in ((4224, 41), (2944, 42)):
        x, y = pair(length, seed)
        loss = ref_cos.CosSimLoss()(torch.from_numpy(x), torch.from_numpy(y))
        out["x_%d" % length], out["y_%d" % length] = x, y
        out["loss_%d" % length] = np.float32(loss.item())
        print(length, float(loss))
    np.savez(os.path.join(HERE, "cos_loss.npz"), **out)
