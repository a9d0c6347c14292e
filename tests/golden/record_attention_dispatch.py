"""Writes tests/golden/attention_short_dispatch.npz: the attention op's output at L = 50 and L = 77 (the whole-sequence MFMA kernels)
for the seeded inputs of tests/test_gpu_clip_towers.py::test_short_sequence_dispatch_is_bit_identical, as computed by the library
that GLASS_LIB names — the build of the commit BEFORE the streaming kernel was added.  Needs a GPU; one process per recording (the
library handle is cached per process).

    GLASS_LIB=/path/to/parent/libglass.so python tests/golden/record_attention_dispatch.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_clip_towers as T  # noqa: E402
from clip_glass_amd import ops  # noqa: E402


def main():
    assert os.environ.get("GLASS_LIB"), "name the recording library with GLASS_LIB"
    out = {}
    for L, causal in T.SHORT_CASES:
        got = ops.attention(T.short_case_input(L), T.SHORT_N_IMG, L, T.SHORT_HEADS, causal)
        half = got.astype(np.float16)
        assert np.array_equal(half.astype(np.float32), got)        # the op returns fp16 values widened to fp32
        out["L%d_causal%d" % (L, int(causal))] = half
    path = sys.argv[1] if len(sys.argv) > 1 else T.SHORT_GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
