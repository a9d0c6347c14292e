"""tests/golden/score_tail_parent.npz: what the diagnostic ops of the score tail (cosine, cosine_views, cosine_set, cosine_set_islands,
cosine_set_dir, assemble_F, assemble_F_set) returned on an MI355X from the library of the commit BEFORE the four cosine kernels and the three
assemble_F kernels became one each (tests/golden/record_score_tail.py).  Outputs only: every test regenerates its inputs from its own seeded
helper.  A case's outputs are stored as one float32 vector, pack(...) of them in the op's order."""
import functools
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_tail_parent.npz")


def pack(*arrays):
    return np.concatenate([np.asarray(a, np.float32).ravel() for a in arrays])


@functools.lru_cache(maxsize=None)
def _file():
    with np.load(PATH) as z:
        return {k: z[k] for k in z.files}


def golden(key):
    return _file()[key]
