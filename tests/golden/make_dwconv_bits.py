"""Records tests/golden/dwconv_bits.json: sha256 of every output and partials tensor of every case of
tests/test_dwconv_bits_gpu.py, as the library in use computes them on the GPU.

It was run ONCE, with the library built from the commit before the depthwise kernels moved into csrc/depthwise.hip and were
built from one window-walk source (TRUNET_HIP_LIB points the package at another build of the library); the test then holds
every later build to those bits.

    TRUNET_HIP_LIB=/path/to/parent/libtrunet_hip.so python tests/golden/make_dwconv_bits.py [OUT.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_dwconv_bits_gpu as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    bits = {}
    for name in T.CASES:
        sha = T.run_case(name)
        assert sha == T.run_case(name), "%s: two runs differ" % name
        assert T.inputs_untouched(name), "%s: an input was written" % name
        bits[name] = sha
    with open(out, "w") as f:
        json.dump(bits, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d cases)" % (out, len(bits)))


if __name__ == "__main__":
    main()
