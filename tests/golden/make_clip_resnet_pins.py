"""Writes tests/golden/clip_resnet_pins.npz: the reference's own ModifiedResNet (clip/model.py build_model -> .visual) on the small tower
cases of tests/clip_resnet_ref.py (build container only), so the float64 restatement stays pinned where the reference is absent.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_clip_resnet_pins.py
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
import test_clip_resnet_ref as T  # noqa: E402


def main():
    assert rh.available(), "needs the reference"
    out = {case: T.ref_visual_features(case) for case in T.R.PIN_CASES}
    np.savez_compressed(T.PINS, **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
