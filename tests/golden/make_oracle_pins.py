"""Writes tests/golden/oracle_pins.npz: the reference's own mini G / D / CLIP modules and clip.tokenize on the inputs of
tests/test_oracle_vs_reference.py (build container only), so those pins hold where the reference is absent.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_oracle_pins.py
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
import test_oracle_vs_reference as T  # noqa: E402


def main():
    assert rh.available(), "needs the reference"
    out = dict(G=T.ref_generator_mini(), D=T.ref_discriminator_mini())
    out["clip_image"], out["clip_text"] = T.ref_clip_mini()
    out["tokens"] = T.ref_tokens()
    np.savez_compressed(os.path.join(HERE, "oracle_pins.npz"), **{k: np.asarray(v) for k, v in out.items()})
    print({k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
