"""conv_down64.hip on the CPU (tests/emu_down64.py): the walk, window / carry / ring / priming / mask indexing.  LDS and the carried rows
are NaN at every priming point, so a finite output equal to the direct computation proves that every stored output read only slots its
own column segment wrote, and the store count proves that every output vector is stored exactly once."""
import numpy as np
import pytest

import emu_down64 as emu
from clip_glass_amd import synth


def _case(B, R, seed=31):
    h16 = lambda a: a.astype(np.float16).astype(np.float32)
    h = h16(synth.normal(seed, "h", (B, R, R, 64)))
    xs = h16(synth.normal(seed, "xs", (B, R // 2, R // 2, 64)))
    w1 = synth.normal(seed, "w1", (128, 64, 3, 3)) / np.float32(24.0)
    ws = synth.normal(seed, "ws", (128, 64, 1, 1)) / np.float32(8.0)
    b1 = synth.normal(seed, "b1", (128,), 0.3)
    return h, xs, w1, ws, b1


@pytest.mark.parametrize("B,R,n_cus", [
    (2, 64, 256),     # 64 steps on 64 workgroups: every step primed; second tile column holds 3 of 29 pixels; all borders
    (1, 64, 5),       # 7-step ranges: priming mid-column, ranges crossing a column boundary, masked tail step on even totals
    (1, 116, 3),      # R/2 = 58: exactly two full tile columns, R % 64 != 0
    (2, 128, 7),      # three tile columns (interior middle one), ranges crossing the sample boundary
])
def test_emulated_kernel_matches_direct(B, R, n_cus):
    h, xs, w1, ws, b1 = _case(B, R)
    stats = {}
    y, count = emu.dblock_down64(h, xs, w1, ws, b1, n_cus=n_cus, stats=stats)
    assert (count == 1).all(), "outputs stored %d..%d times" % (count.min(), count.max())
    assert np.isfinite(y).all(), "%d outputs read unwritten LDS / carry" % (~np.isfinite(y)).sum()
    ref = emu.reference(h, xs, w1, ws, b1)
    # same fp16 FIR values on both sides: what is left is the fp32 accumulation order and the fp16 rounding of the output
    err = np.abs(y - ref).max()
    assert err <= 2.0 ** -10 * max(1.0, np.abs(ref).max()), err
    assert stats["primes"] >= stats["grid"]


def test_walk_counts():
    """total = real steps + one priming step per column segment, for every split of a small problem."""
    tiles_x, SY, B = 2, 16, 2
    steps = B * tiles_x * SY
    for n_cus in range(1, steps + 1):
        per_block = (steps + n_cus - 1) // n_cus
        seen = []
        for first in range(0, steps, per_block):
            last = min(first + per_block, steps)
            w = emu._Walk(first, last, tiles_x, SY)
            out = [w.issue() for _ in range(w.total)]
            real = [(o["b"], o["tx"], o["s"]) for o in out if o["valid"]]
            assert len(real) == last - first and w.left == 0 and not w.prime
            prev = None
            for o in out:       # every real step follows the step above it in the same column (real or priming)
                if o["valid"]:
                    assert prev is not None and (prev["b"], prev["tx"], prev["s"]) == (o["b"], o["tx"], o["s"] - 1)
                prev = o
            assert all(not o["valid"] and not o["prime"] for o in [w.issue(), w.issue()])     # padding steps are masked
            seen += real
        assert seen == [(b, tx, s) for b in range(B) for tx in range(tiles_x) for s in range(SY)]


def test_gate():
    assert emu.gate(512, 64, 128) and emu.gate(116, 64, 128) and emu.gate(16, 64, 128)
    assert not emu.gate(512, 32, 64) and not emu.gate(256, 128, 256) and not emu.gate(66, 64, 128) and not emu.gate(8, 64, 128)
