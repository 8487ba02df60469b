"""GPU: the order of the profiled launches of one training step, per engine and per fusion toggle, against the trace
recorded before the two engines were given one schedule source (tests/golden/engine_launch_trace.json, written by
tests/golden/make_engine_launch_trace.py).  Equal outputs prove equal arithmetic; the trace proves that no launch was
added, dropped, reordered or moved between the fused and the separate path."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_schedule_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu


def _diff(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return "launch %d: got %s, recorded %s" % (i, a, b)
    return "%d launches, recorded %d" % (len(got), len(want))


@pytest.mark.parametrize("name", list(S.CASES))
def test_launch_trace_of_a_training_step(name, monkeypatch):
    with open(S.GOLDEN) as f:
        want = json.load(f)[name]
    bf16 = S.CASES[name][0]
    traces = S.run_case(name, monkeypatch.setattr, steps=2 if bf16 else 1)
    assert want
    assert traces[0] == want, _diff(traces[0], want)
    if bf16:        # from the second step on the weight images come from the batched pack
        assert traces[1] == traces[0], _diff(traces[1], traces[0])
