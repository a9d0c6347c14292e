"""Writes tests/golden/score_tail_parent.npz: the outputs of the score tail's diagnostic ops (cosine, cosine_views, cosine_set,
cosine_set_islands, cosine_set_dir, assemble_F, assemble_F_set) at the shapes of their tests, as computed by the library that GLASS_LIB
names — the build of the commit BEFORE csrc/score.hip, where cosine_kernel, cosine_views_kernel, cosine_set_kernel, cosine_set_dir_kernel and
the three assemble_F kernels were separate.  Outputs only: the inputs are the tests' own seeded helpers.  Needs a GPU; one process.

    GLASS_LIB=/path/to/parent/libglass.so python tests/golden/record_score_tail.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import edit_ref as E  # noqa: E402
import test_gpu_edit_ops as TE  # noqa: E402
import test_gpu_islands_ops as TI  # noqa: E402
import test_gpu_prompt_set_ops as TP  # noqa: E402
import test_gpu_small_ops as TS  # noqa: E402
from clip_glass_amd import ops  # noqa: E402
from score_tail_golden import PATH, pack  # noqa: E402


def main():
    assert os.environ.get("GLASS_LIB"), "name the recording library with GLASS_LIB"
    out = {}
    for D in TS.COSINE_D:
        out["cosine_D%d" % D] = pack(ops.cosine(*TS._cosine_case(D)))
    for V in TS.COSINE_VIEWS_V:
        out["cosine_views_V%d" % V] = pack(*ops.cosine_views(*TS._cosine_views_case(V)))
    for P in TS.ASSEMBLE_F_P:
        for n_obj in (1, 2):
            out["assemble_F_P%d_n%d" % (P, n_obj)] = pack(ops.assemble_F(*TS._assemble_F_case(P, n_obj)))
    shapes = [(TP.P, V, T, D) for D in TP.SET_D for V in TP.SET_V for T in TP.SET_T] + [TP.STREAMED] + TP.EDGES
    for shape in shapes:
        out["cosine_set_P%d_V%d_T%d_D%d" % shape] = pack(*ops.cosine_set(*TP._inputs(*shape)))
    for Pn in TP.F_SET_P:
        for K in TP.F_SET_K:
            for has_d, has_lp in TP.F_SET_COLS:
                out["assemble_F_set_P%d_K%d_d%d_lp%d" % (Pn, K, has_d, has_lp)] = pack(ops.assemble_F_set(*TP._assemble_F_set_case(Pn, K, has_d, has_lp)))
    for V in TI.ISLAND_V:
        out["island_cosine_V%d" % V] = pack(*ops.cosine_set_islands(*TI._island_cosine_case(V)))
    for D in TE.DIR_D:
        for T in TE.DIR_T:
            staged, streamed = [], []
            for V in TE.DIR_V:
                for P in TE.DIR_P:
                    case = E.dir_inputs(P, V, T, D)
                    staged += ops.cosine_set_dir(*case)
                    streamed += ops.cosine_set_dir(*case, streamed=True)
            a, b = pack(*staged), pack(*streamed)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (D, T)      # one vector stands for both forms
            out["cosine_set_dir_D%d_T%d" % (D, T)] = a
    for k, v in out.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", sum(v.size for v in out.values()), "values,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
