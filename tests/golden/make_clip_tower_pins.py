"""Writes tests/golden/clip_tower_pins.npz: the reference's own CLIP image tower (clip/model.py build_model -> .visual) on the
inputs of tests/test_clip_geometry.py at patch 16 / res 64 and patch 14 / res 56 (build container only), so the oracle's pin at
those patch sizes holds where the reference is absent.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_clip_tower_pins.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import ref_harness as rh  # noqa: E402
import test_clip_geometry as T  # noqa: E402


def main():
    assert rh.available(), "needs the reference"
    out = {T.pin_name(patch, res): T.ref_encode_image(patch, res) for patch, res in T.ORACLE_CASES}
    np.savez_compressed(T.PINS, **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
