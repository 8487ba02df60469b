"""Records tests/golden/engine_launch_trace.json: the ordered (kernel family, tag) list of the profiled launches of one
training step, for every case of tests/engine_schedule_cases.py, on the GPU.

It was run ONCE, at the commit before the fp32 and bf16 engines were given one schedule source;
tests/test_engine_schedule_gpu.py holds every later schedule to that order.

    python tests/golden/make_engine_launch_trace.py [OUT.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import engine_schedule_cases as S  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else S.GOLDEN
    doc = {}
    for name in S.CASES:
        undo = []

        def set_off(mod, attr, value):
            undo.append((mod, attr, getattr(mod, attr)))
            setattr(mod, attr, value)
        try:
            first, second = S.run_case(name, set_off, steps=2)
        finally:
            for mod, attr, old in reversed(undo):
                setattr(mod, attr, old)
        assert first == second, "%s: the second step launches differently from the first" % name
        doc[name] = first
        print("%-20s %d launches" % (name, len(first)))
    with open(out, "w") as f:          # one launch per line
        f.write("{\n" + ",\n".join("%s: [\n%s\n]" % (json.dumps(name), ",\n".join(" " + json.dumps(r) for r in trace))
                                  for name, trace in doc.items()) + "\n}\n")
    print("wrote %s" % out)


if __name__ == "__main__":
    main()
