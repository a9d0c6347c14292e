"""A conv family refuses what its kernel does not implement — by name, never by dropping it.

Every `impl` of ops.conv asks one family (or a short list) through the family's chooser (csrc/kernels.h).  The table below says, per family,
which of the launch features ops.conv can express lie OUTSIDE what its kernel reads; it is written by hand from the kernels, not taken from
the library.  Each such feature must raise RuntimeError with the family and the feature in the message.  The chooser decides on the host and no
conv kernel is launched (the op still uploads its operands and runs its small set-up kernels, the toRGB tables and the weight modulation,
before it asks), so the cases cost milliseconds.  B = 1, 32 x 32, 64 -> 64 channels (128 -> 128 for conv_glds, whose geometry
starts there, and for the toRGB partial sums, which need a 128-wide n tile).

Not expressible through ops.conv, so not here: the fp32 output, the fused fromRGB input, a broadcast input at B = 1."""
import re

import numpy as np
import pytest

from clip_glass_amd import ops

pytestmark = pytest.mark.gpu

B, H, W = 1, 32, 32


def _case(C):
    rng = np.random.default_rng(C)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x, w = f(B, H, W, C), f(C, C, 3, 3) * 0.05
    torgb = dict(w=f(3, C), b=f(3), sn=f(B, C), smax=np.ones(B, np.float32))
    # feature -> (ops.conv arguments, the feature's name in a refusal)
    feats = {
        "up": (dict(up=True), "[up]"),
        "sn": (dict(sn=f(B, C)), "[sn "),
        "pre_shift": (dict(sn=f(B, C), pre_shift=f(B, C)), "[pre_shift]"),
        "in_up": (dict(in_up=True), "[in_up]"),
        "dscale": (dict(dscale=f(B, C)), "[dscale]"),
        "shift": (dict(shift=f(B, C)), "[shift]"),
        "noise": (dict(noise=f(B, H, W), noise_strength=0.1), "[noise]"),
        "res": (dict(res=f(B, H, W, C)), "[res]"),
        "res_cs": (dict(res=f(B, H, W, C + 8), res_cs=C + 8), "[res_cs]"),
        "res_up": (dict(res=f(B, H // 2, W // 2, C), res_up=True), "[res_up]"),
        "premod": (dict(sn=f(B, C), premod=True), "[premod "),
        "torgb": (dict(torgb=torgb, both=True), "[trgb_yout (fused toRGB)]"),
        "trgb_partial": (dict(torgb=torgb, both=True, trgb_partial=True), "[trgb_partial]"),
        "rgb_tanh": (dict(rgb_tanh=True), "[rgb_tanh"),
        "xs_out": (dict(xs_out=np.zeros((B, H // 2, W // 2, C), np.float32)), "[xs_out]"),
        "post_scale": (dict(post_scale=f(B, C)), "[post_scale]"),
        "skip": (dict(skip=(f(B, H, W, C), f(C, C, 1, 1))), "[skip_x "),
        "planar_x": (dict(planar_x=True), "[x_planar8]"),
        "planar_y": (dict(planar_y=True), "[y_planar8]"),
        "planar32_x": (dict(planar32_x=True), "[x_planar32]"),
    }
    return x, w, feats


# (id, impl, family named in the refusal, channels, arguments every call of the row carries, features OUTSIDE the family's mask)
_DIRECT_LIKE = ["premod", "torgb", "trgb_partial", "rgb_tanh", "xs_out", "post_scale", "skip", "planar_x", "planar_y", "planar32_x"]
ROWS = [
    # conv_direct_kernel reads: up, sn, pre_shift, in_up, dscale, shift, noise, res (res_cs, res_up)
    ("direct", 1, "conv_direct", 64, {}, _DIRECT_LIKE),
    # conv_tiled_kernel adds per-sample weights, toRGB in the epilogue, the planar tanh, xs_out and the fused skip
    ("tiled", 2, "conv_tiled", 64, {}, ["trgb_partial", "post_scale", "planar_x", "planar_y", "planar32_x"]),
    # upfir2_kernel reads: up, sn16, dscale, noise, per-sample weights, post_scale, y_planar8
    ("upfir", 3, "upfir", 64, {}, ["pre_shift", "in_up", "shift", "res", "res_cs", "res_up", "torgb", "trgb_partial", "rgb_tanh", "xs_out", "skip",
                                   "planar_x", "planar32_x"]),
    # conv_stream_kernel reads: sn16, dscale, shift, noise, per-sample weights, (fromRGB,) toRGB INSTEAD of the map
    ("stream", 4, "conv_stream", 64, {}, ["up", "pre_shift", "in_up", "res", "res_cs", "res_up", "trgb_partial", "rgb_tanh", "xs_out", "post_scale",
                                          "skip", "planar_x", "planar_y", "planar32_x"]),
    # conv_wreg_kernel reads: dscale, shift, noise, per-sample weights, toRGB, xs_out, x_planar8
    ("wreg", 5, "conv_wreg", 64, {}, ["up", "sn", "pre_shift", "in_up", "res", "res_cs", "res_up", "trgb_partial", "rgb_tanh", "post_scale",
                                      "planar_y", "planar32_x"]),
    # conv_glds_kernel / conv_gldsp_kernel read: sn16, dscale, shift, noise, res (res_cs, res_up), per-sample weights, toRGB, its partial sums, xs_out
    ("glds", 5, "conv_glds", 128, {}, ["up", "pre_shift", "in_up", "rgb_tanh", "post_scale", "planar_x", "planar_y", "planar32_x"]),
    # conv_s2_kernel (impl 5 with the skip operands) reads: skip_x / skip_w, x_planar32 — and nothing else
    ("s2", 5, "conv_s2", 64, "skip", ["up", "sn", "pre_shift", "in_up", "dscale", "shift", "noise", "res", "res_cs", "res_up", "premod", "torgb",
                                      "trgb_partial", "rgb_tanh", "xs_out", "post_scale", "planar_x", "planar_y"]),
    # conv_im2col_kernel + conv_finish_kernel read what conv_direct_kernel reads
    ("gemm", 6, "conv_gemm", 64, {}, _DIRECT_LIKE),
    # impl 0 asks conv_stream, conv_s2, conv_tiled, conv_direct (upfir first for an up-conv): what none of them implements;
    # x_planar32 is conv_s2's, which wants the skip operands with it
    ("auto", 0, "conv_direct", 64, {}, ["trgb_partial", "post_scale", "planar_x", "planar_y", "planar32_x"]),
]
CASES = [(rid, impl, family, C, base, feat) for rid, impl, family, C, base, feats in ROWS for feat in feats]


@pytest.mark.parametrize("rid,impl,family,C,base,feat", CASES, ids=["%s-%s" % (c[0], c[5]) for c in CASES])
def test_family_refuses_feature_outside_its_mask(rid, impl, family, C, base, feat):
    if feat == "trgb_partial":
        C = 128                                           # (one 128-wide n tile per partial sum)
    x, w, feats = _case(C)
    kw, name = feats[feat]
    kw = dict(kw)
    if base == "skip":
        kw.update(feats["skip"][0])
    if "in_up" in kw:
        x = x[:, :H // 2, :W // 2]                        # the stored map; H x W are the upsampled dims
    with pytest.raises(RuntimeError, match=re.escape(family) + r" does not implement[^;]*" + re.escape(name)):
        ops.conv(x, w, impl=impl, **kw)


def test_stream_refuses_torgb_beside_a_stored_map():
    """conv_stream<torgb> writes the skip image INSTEAD of the feature map: asked for both, it refuses (it used to take the launch and leave
    y unwritten).  Without the map the same launch runs."""
    x, w, feats = _case(32)
    Hs, Ws = 64, 512                                      # a map conv_stream takes: 64 nominal candidates x (W / 32)(H / 8) tiles >= 6 per slot
    x = np.random.default_rng(1).standard_normal((B, Hs, Ws, 32)).astype(np.float32)
    torgb = feats["torgb"][0]["torgb"]
    with pytest.raises(RuntimeError, match=r"conv_stream does not take this shape or this combination of[^;]*\[trgb_yout \(fused toRGB\)\]"):
        ops.conv(x, w, impl=4, torgb=torgb, both=True)
    y = ops.conv(x, w, impl=4, torgb=torgb)
    assert y.shape == (B, 3, Hs, Ws) and np.isfinite(y).all()
