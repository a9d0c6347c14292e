"""ctypes binding of the diagnostic per-kernel ABI (include/glass_ops.h).

Used by tests/ to check each HIP kernel family against the oracle in isolation.
Activations are NHWC float32 on the host; conversion to the kernels' fp16 layouts
happens inside the library.
"""
import ctypes as C

import numpy as np

from .engine import _check, _f32, _fp, bind, load_library


class ConvDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32),
                ("KS", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32), ("up", C.c_int32),
                ("Ho", C.c_int32), ("Wo", C.c_int32), ("broadcast_x", C.c_int32), ("act", C.c_int32),
                ("batch_size", C.c_int32), ("impl", C.c_int32),
                ("noise_strength", C.c_float), ("out_scale", C.c_float),
                ("x", C.POINTER(C.c_float)), ("w", C.POINTER(C.c_float)), ("sn", C.POINTER(C.c_float)),
                ("dscale", C.POINTER(C.c_float)), ("noise", C.POINTER(C.c_float)), ("bias", C.POINTER(C.c_float)),
                ("res", C.POINTER(C.c_float)), ("y", C.POINTER(C.c_float)),
                ("trgb_w", C.POINTER(C.c_float)), ("trgb_b", C.POINTER(C.c_float)), ("trgb_sn", C.POINTER(C.c_float)),
                ("trgb_smax", C.POINTER(C.c_float)), ("trgb_yprev", C.POINTER(C.c_float)),
                ("trgb_yout", C.POINTER(C.c_float)),
                ("skip_x", C.POINTER(C.c_float)), ("skip_w", C.POINTER(C.c_float)), ("xs_out", C.POINTER(C.c_float)),
                ("x_planar8", C.c_int32), ("x_planar32", C.c_int32),
                ("premod", C.c_int32), ("post_scale", C.POINTER(C.c_float)), ("y_planar8", C.c_int32),
                ("trgb_partial", C.c_int32),
                ("pre_shift", C.POINTER(C.c_float)), ("in_up", C.c_int32), ("shift", C.POINTER(C.c_float)),
                ("res_cs", C.c_int32), ("res_up", C.c_int32), ("rgb_tanh", C.POINTER(C.c_float)), ("trgb_keep_map", C.c_int32)]


# The C signature of every function of include/glass_ops.h, argument by argument (all return int32).  _lib() sets them once;
# tests/test_ops_signatures.py holds this table and ConvDesc against the header.
i32, u32, i64, u64, f32, f64 = C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_float, C.c_double
fp, ip, dp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
SIGNATURES = {
    "glass_op_conv": [i32, C.POINTER(ConvDesc)],
    "glass_op_gemm": [i32, i32, i32, i32, fp, fp, fp, i32, i32, fp],
    "glass_op_gemm_batched": [i32, i32, i32, i32, i32, fp, fp, i32, i32, i32, fp],
    "glass_op_gemm_ex": [i32, i32, i32, i32, i32, i32, fp, fp, fp, i32, i32, i32, i32, fp, C.c_char_p, i32],
    "glass_op_dense": [i32, i32, i32, i32, fp, fp, fp, i32, i32, fp, fp],
    "glass_op_torgb": [i32, i32, i32, i32, fp, fp, fp, fp, fp, fp, fp],
    "glass_op_blur": [i32, i32, i32, i32, i32, fp, fp],
    "glass_op_dblock_down": [i32, i32, i32, i32, i32, fp, fp, fp, fp, fp, fp],
    "glass_op_dblock0": [i32, i32, i32, i32, fp, fp, fp, fp, fp, fp, fp, fp, fp],
    "glass_op_last_kernel": [C.c_char_p, i32],
    "glass_op_fromrgb": [i32, i32, i32, i32, fp, fp, fp, fp],
    "glass_op_mbstd": [i32, i32, i32, i32, i32, i32, i32, fp, fp],
    "glass_op_resize": [i32, i32, i32, i32, i32, fp, fp],
    "glass_op_view_patches": [i32, i32, i32, i32, i32, i32, i32, ip, fp, fp],
    "glass_op_preprocess": [i32, i32, i32, i32, i32, i32, i32, fp, fp],
    "glass_op_layernorm": [i32, i32, i32, fp, fp, fp, fp],
    "glass_op_attention": [i32, i32, i32, i32, i32, fp, fp],
    "glass_op_noise": [i32, i32, i32, u32, u32, u32, u64, fp],
    "glass_op_noise_period": [i32, i32, i32, u32, u32, u32, u64, u32, fp],
    "glass_op_gpt2_sample": [i32, i32, i32, fp, f32, i32, u64, i32, i32, i32, i32, ip],
    "glass_op_gpt2_gemm": [i32, i32, i32, i32, i32, i32, i32, i32, fp, fp, fp, fp, fp, fp, i32, fp, fp, fp, ip],
    "glass_op_gpt2_attention": [i32, i32, i32, i32, i32, i32, i32, i32, fp, fp, fp, fp, fp],
    "glass_op_gpt2_head": [i32, i32, i32, i32, i32, fp, fp, fp, fp, fp, i32, i32, i32, fp, fp, ip, ip, fp, fp, fp, ip],
    "glass_op_gpt2_embed_step": [i32, i32, i32, i32, ip, fp, fp, i32, i32, i32, fp, fp],
    "glass_op_bg_cond": [i32, i32, i32, i32, i32, fp, fp, fp],
    "glass_op_bg_bn_tables": [i32, i32, i32, i32, fp, fp, fp, fp, fp, fp, fp, fp],
    "glass_op_bg_attn_split": [i32, i32, i32, i32, i32, i32, fp, fp, fp, fp, ip],
    "glass_op_bg_softmax": [i32, i32, i32, fp, fp],
    "glass_op_bg_rgb_tanh": [i32, i32, i32, i32, fp, fp],
    "glass_op_bg_to_half": [i32, i64, fp, fp],
    "glass_op_bg_tail": [i32, i32, i32, i32, fp, fp, fp, fp, fp, fp, fp, fp, fp],
    "glass_op_rn_avgpool": [i32, i32, i32, i32, i32, fp, fp],
    "glass_op_rn_stem_conv1": [i32, i32, i32, i32, fp, fp, fp, fp, fp],
    "glass_op_rn_conv_bn": [i32, i32, i32, i32, i32, i32, i32, i32, i32, fp, fp, fp, fp, fp, fp],
    "glass_op_rn_tokens": [i32, i32, i32, i32, fp, fp, fp],
    "glass_op_mapping": [i32, i32, i32, i32, fp, fp, fp, i32, fp, ip],
    "glass_op_pixelnorm": [i32, i32, i32, fp, fp],
    "glass_op_dense_splitk": [i32, i32, i32, i32, i32, i32, i32, fp, fp, fp, fp],
    "glass_op_dense_ex": [i32, i32, i32, i32, i32, i32, fp, fp, fp, i32, i32, fp, i32, fp],
    "glass_op_dense_multi": [i32, i32, i32, i32, i32, i32, ip, ip, ip, ip, ip, fp, fp, fp, fp],
    "glass_op_style_norm": [i32, i32, i32, i32, ip, ip, fp, fp, fp],
    "glass_op_d_head": [i32, i32, i32, fp, fp, fp, fp, fp, fp, ip],
    "glass_op_finalize_image": [i32, i64, fp, fp],
    "glass_op_embed_lnpre": [i32, i32, i32, i32, fp, fp, fp, fp, fp, fp],
    "glass_op_embed_text": [i32, i32, i32, i32, i32, ip, fp, fp, fp],
    "glass_op_layernorm_ex": [i32, i32, i32, i64, i32, fp, fp, fp, fp],
    "glass_op_layernorm_rows": [i32, i32, i32, i32, fp, ip, fp, fp, fp],
    "glass_op_cosine": [i32, i32, i32, fp, fp, fp],
    "glass_op_cosine_views": [i32, i32, i32, i32, fp, fp, fp, fp],
    "glass_op_assemble_F": [i32, i32, i32, fp, fp, fp],
    "glass_op_cosine_set": [i32, i32, i32, i32, i32, fp, fp, fp, fp, fp, fp],
    "glass_op_cosine_set_islands": [i32, i32, i32, i32, i32, fp, fp, fp, i32, i32, i32, fp, fp, fp],
    "glass_op_assemble_F_set": [i32, i32, i32, fp, fp, fp, fp, fp],
    "glass_op_cosine_set_dir": [i32, i32, i32, i32, i32, fp, fp, fp, fp, i32, fp, fp, fp],
    "glass_op_latent_anchor": [i32, i32, i32, i32, i32, fp, fp, fp],
    "glass_op_dlatent_subspace": [i32, fp, i32, i32, i32, ip, i32, i32, fp, fp, fp],
    "glass_op_image_patches": [i32, i32, i32, i32, i32, fp, f32, fp],
    "glass_op_rn_token0_rows": [i32, i32, i32, i32, fp, fp],
    "glass_op_lpips_input": [i32, i32, i32, i32, fp, fp],
    "glass_op_vgg_conv1": [i32, i32, i32, fp, fp, fp, fp],
    "glass_op_maxpool2": [i32, i32, i32, i32, i32, fp, fp],
    "glass_op_lpips_head": [i32, i32, i32, i32, i32, fp, fp, fp, fp],
    "glass_op_ga_vary": [i32, i32, i32, fp, ip, dp, f64, f64, f64, f64, f64, u64, i32, i32, i32, fp],
    "glass_op_ga_vary_mixed": [i32, i32, i32, i32, fp, ip, dp, f64, f64, f64, f64, f64, f64, f64, u64, i32, i32, i32, fp],
    "glass_op_ga_duplicates": [i32, i32, i32, i32, fp, fp, ip],
    "glass_op_ga_survive": [i32, i32, i32, i32, i32, i32, fp, ip, ip, ip, dp, fp, ip, i32, fp, fp, fp],
    "glass_op_ga_migrate": [i32, i32, i32, i32, i32, i32, i32, fp, fp, ip, dp, fp, fp, ip, dp, ip],
    "glass_op_cma_sample": [i32, i32, i32, dp, dp, f64, f64, f64, u64, i32, i32, i32, fp],
    "glass_op_cma_rank": [i32, i32, fp, f32, ip, ip, fp],
    "glass_op_cma_update": [i32, i32, i32, fp, fp, dp, dp, ip, f64, f64, i32, fp, fp, ip],
    "glass_op_mfma_probe": [i32, fp, fp, fp],
    "glass_host_pack_conv": [fp, i32, i32, i32, i32, fp],
    "glass_host_resize_taps": [i32, i32, i32, ip, ip, fp, i32],
    "glass_host_gpt2_gemm_choice": [i32, i32, i32, i32, i32, i32, i32, ip, ip],
    "glass_host_gpt2_step_plan": [i32, i32, i32, i32, i32, i32, i32, C.c_char_p, i32],
}
_signed = None      # the library SIGNATURES was last applied to


def _lib():
    """load_library() with SIGNATURES applied (a second build loaded through GLASS_LIB may lack the newer functions)."""
    global _signed
    lib = load_library()
    if lib is not _signed:
        bind(lib, SIGNATURES)
        _signed = lib
    return lib


def to_planar8(a):
    """[B,H,W,C] -> the chunk-planar layout [B,C/8,H,W,8] conv_wreg's producers write (csrc/common.h x_planar8)."""
    B, H, W, Cc = a.shape
    return np.ascontiguousarray(a.reshape(B, H, W, Cc // 8, 8).transpose(0, 3, 1, 2, 4))


def to_planar32(a):
    """[B,H,W,C] -> 32-channel planes [B,C/32,H,W,32]: the layout the pad-2 blur writes for conv_s2 (csrc/common.h x_planar32)."""
    B, H, W, Cc = a.shape
    return np.ascontiguousarray(a.reshape(B, H, W, Cc // 32, 32).transpose(0, 3, 1, 2, 4))


def from_planar32(a, B, H, W, Cc):
    return np.ascontiguousarray(a.reshape(B, Cc // 32, H, W, 32).transpose(0, 2, 3, 1, 4)).reshape(B, H, W, Cc)


def from_planar8(a, B, H, W, Cc):
    return np.ascontiguousarray(a.reshape(B, Cc // 8, H, W, 8).transpose(0, 2, 3, 1, 4)).reshape(B, H, W, Cc)


def _opt(a):
    if a is None:
        return None, None
    a = _f32(a)
    return a, _fp(a)


def conv(x, w, *, stride=1, pad=None, up=False, sn=None, dscale=None, noise=None, noise_strength=0.0,
         batch_size=1, bias=None, act=False, res=None, out_scale=1.0, impl=0, broadcast_x=False, B=None, device=0,
         torgb=None, skip=None, xs_out=None, planar_x=False, both=False, planar32_x=False, premod=False, post_scale=None,
         planar_y=False, trgb_partial=False, pre_shift=None, in_up=False, shift=None, res_cs=0, res_up=False, rgb_tanh=False):
    """x [B,H,W,Cin] NHWC; w [Cout,Cin,KS,KS] (reference layout).  Returns y [B,Ho,Wo,Cout].
    torgb = dict(w [3,Cout], b [3], sn [B,Cout], smax [B], yprev [B,3,Ho/2,Wo/2] or None) with impl=4: the fused conv + toRGB
    form of the streaming kernel — returns the skip image [B,3,Ho,Wo] instead of y (with both=True it is asked for the map too, and refuses).
    planar_x: the device gets x chunk-planar (the permutation happens here; impl 5, 64 -> 64).
    The forms the StyleGAN2 host builds (csrc/stylegan2.cpp): premod — sn / dscale go into per-sample weights first
    (modulate_weights_kernel) and the conv runs without them; post_scale [B,Cout] — the consumer's style applied to the finished
    output (fused up-conv); planar_y — the device stores y chunk-planar (un-permuted here); trgb_partial — with torgb and impl 5: toRGB
    partial sums per 128-wide n tile + the finishing pass.
    The forms the BigGAN host builds (csrc/biggan.cpp bg_conv): pre_shift [B,Cin] with sn — relu(x * sn + pre_shift) while staging, the zero
    padding stays zero; in_up — x is [B,H/2,W/2,Cin], read through a nearest x2 upsample; shift [B,Cout] — added after the bias (act=2:
    ReLU); res [B,Ho >> res_up,Wo >> res_up,res_cs or Cout] — the first Cout channels, nearest x2 with res_up; rgb_tanh — returns
    tanh(channels 0..2) [B,3,Ho,Wo] from the accumulators instead of y (conv_tiled only)."""
    lib = _lib()
    x = _f32(x); w = _f32(w)
    Bx, H, W, Cin = x.shape
    if in_up:
        H, W = 2 * H, 2 * W
    if planar_x:
        x = to_planar8(x)
    if planar32_x:            # conv_s2's input in 32-channel planes (permuted here)
        x = to_planar32(x)
    B = B if B is not None else Bx
    Cout, _, KS, _ = w.shape
    pad = (KS // 2) if pad is None else pad
    if up:
        Ho, Wo = 2 * H, 2 * W
    else:
        Ho, Wo = (H + 2 * pad - KS) // stride + 1, (W + 2 * pad - KS) // stride + 1
    y = np.full((B, Ho, Wo, Cout), np.nan, dtype=np.float32)      # (NaN: what the op does not fetch shows)
    d = ConvDesc()
    d.B, d.H, d.W, d.Cin, d.Cout = B, H, W, Cin, Cout
    d.KS, d.stride, d.pad, d.up, d.Ho, d.Wo = KS, stride, pad, int(up), Ho, Wo
    d.broadcast_x, d.act, d.batch_size, d.impl = int(broadcast_x), int(act), batch_size, impl
    d.noise_strength, d.out_scale = noise_strength, out_scale
    d.x_planar8 = int(planar_x)
    d.x_planar32 = int(planar32_x)
    d.premod, d.y_planar8, d.trgb_partial = int(premod), int(planar_y), int(trgb_partial)
    d.in_up, d.res_cs, d.res_up = int(in_up), int(res_cs), int(res_up)
    d.trgb_keep_map = int(both)     # (impl 4 writes the skip image INSTEAD of the map: with both it refuses)
    keep = []
    d.x, d.w, d.y = _fp(x), _fp(w), _fp(y)
    for name, val in (("sn", sn), ("dscale", dscale), ("noise", noise), ("bias", bias), ("res", res), ("post_scale", post_scale),
                      ("pre_shift", pre_shift), ("shift", shift)):
        a, p = _opt(val)
        keep.append(a)
        if p is not None:
            setattr(d, name, p)
    if skip is not None:      # (skip_x [B,Ho,Wo,Cin], skip_w [Cout,Cin,1,1]): the D block's 1x1 skip conv fused as extra K stages
        for name, val in zip(("skip_x", "skip_w"), skip):
            a, p = _opt(val)
            keep.append(a)
            setattr(d, name, p)
    if xs_out is not None:    # float32 [B,H/2,W/2,Cin] array that receives the blur-down by-product (impl 2, 64 -> 64)
        d.xs_out = _fp(xs_out)
    yrgb = None
    if torgb is not None:
        yrgb = np.full((B, 3, Ho, Wo), np.nan, dtype=np.float32)
        for name in ("w", "b", "sn", "smax", "yprev"):
            a, p = _opt(torgb.get(name))
            keep.append(a)
            if p is not None:
                setattr(d, "trgb_" + name, p)
        d.trgb_yout = _fp(yrgb)
    ytanh = None
    if rgb_tanh:
        ytanh = np.full((B, 3, Ho, Wo), np.nan, dtype=np.float32)
        d.rgb_tanh = _fp(ytanh)
    _check(lib, lib.glass_op_conv(device, C.byref(d)))
    if rgb_tanh:
        return ytanh
    if planar_y:
        y = from_planar8(y, B, Ho, Wo, Cout)
    if both:                  # fused toRGB forms that store the feature map too (impl 2 / 5): (skip image, feature map)
        return yrgb, y
    return yrgb if yrgb is not None else y


def last_kernel():
    """The kernel symbol(s) the last conv / dblock_down / dblock0 of this thread launched ("a + b" for two launches; "" for none) — and of the
    last rn_avgpool, rn_stem_conv1 (the conv itself, not the patch operand's preparation), rn_conv_bn, rn_tokens, lpips_input, vgg_conv1 or
    maxpool2, and of the last gemm, gemm_batched or bg_tail."""
    lib = _lib()
    buf = C.create_string_buffer(512)
    _check(lib, lib.glass_op_last_kernel(buf, len(buf)))
    return buf.value.decode()


def gemm(a, w, bias=None, mode=3, impl=0, acc=None, device=0):
    lib = _lib()
    a = _f32(a); w = _f32(w)
    M, K = a.shape
    N = w.shape[0]
    out = _f32(acc).copy() if acc is not None else np.empty((M, N), dtype=np.float32)
    b, bp = _opt(bias)
    _check(lib, lib.glass_op_gemm(device, M, N, K, _fp(a), _fp(w), bp, mode, impl, _fp(out)))
    return out


def gemm_batched(a, w, mode=3, cand_batch=True, impl=0, device=0):
    """a [batch,M,K], w [batch,N,K] -> out [batch,M,N] = a[z] @ w[z]^T, set up as the BigGAN self-attention products (csrc/biggan.cpp
    bg_attention).  mode 3: fp32 out, 0: fp16 out.  impl 0: gemm_tiled, then gemm_direct where it refuses; 1: direct; 2: tiled."""
    lib = _lib()
    a = _f32(a); w = _f32(w)
    batch, M, K = a.shape
    N = w.shape[1]
    assert w.shape == (batch, N, K)
    out = np.empty((batch, M, N), dtype=np.float32)
    _check(lib, lib.glass_op_gemm_batched(device, batch, M, N, K, _fp(a), _fp(w), int(mode), int(cand_batch), int(impl), _fp(out)))
    return out


def gemm_ex(a, w, out, bias=None, mode=3, impl=2, cand_rows=0, cand_batch=False, device=0):
    """a [M,K] / [batch,M,K], w [N,K] / [batch,N,K], bias [N] -> the name of the kernel that ran, exactly as the launcher returned it.  out
    [M,ldo] / [batch,M,ldo] (C-contiguous float32, ldo >= N) is written IN PLACE: the device output is preloaded from it, so mode 2's
    accumulator, the ldo padding and the caller's sentinels come back as the kernel left them — also when the call raises on a refusal.
    impl 0: gemm_tiled, then gemm_direct where it refuses; 1: gemm_direct; 2: gemm_tiled, a refusal raises.  cand_rows / cand_batch: GemmParams'."""
    lib = _lib()
    a = _f32(a); w = _f32(w)
    if a.ndim == 2:
        a, w = a[None], w[None]
    batch, M, K = a.shape
    N = w.shape[1]
    assert w.shape == (batch, N, K)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.flags.writeable
    assert out.ndim >= 2 and out.size == batch * M * out.shape[-1], "out must be [batch, M, ldo]"
    b, bp = _opt(bias)
    assert b is None or b.shape == (N,)
    name = C.create_string_buffer(128)
    _check(lib, lib.glass_op_gemm_ex(device, batch, M, N, K, out.shape[-1], _fp(a), _fp(w), bp, int(mode), int(impl), int(cand_rows),
                                     int(bool(cand_batch)), _fp(out), name, len(name)))
    return name.value.decode()


def dense(x, wt, bias=None, in_sq=False, mode=0, eps_row=None, device=0):
    lib = _lib()
    x = _f32(x); wt = _f32(wt)
    P, K = x.shape
    N = wt.shape[1]
    out = np.empty((P, N), dtype=np.float32)
    b, bp = _opt(bias)
    e, ep = _opt(eps_row)
    _check(lib, lib.glass_op_dense(device, P, K, N, _fp(x), _fp(wt), bp, int(in_sq), mode, ep, _fp(out)))
    return out


def torgb(x, wrgb, bias, sn, smax, yprev=None, device=0):
    lib = _lib()
    x = _f32(x)
    B, H, _, Cc = x.shape
    wrgb, bias, sn, smax = _f32(wrgb), _f32(bias), _f32(sn), _f32(smax)
    yp, ypp = _opt(yprev)
    out = np.empty((B, 3, H, H), dtype=np.float32)
    _check(lib, lib.glass_op_torgb(device, B, H, Cc, _fp(x), _fp(wrgb), _fp(bias), _fp(sn), _fp(smax), ypp, _fp(out)))
    return out


def blur(x, mode, device=0):
    lib = _lib()
    x = _f32(x)
    B, H, _, Cc = x.shape
    Ho = H + 1 if mode != 1 else H // 2      # mode 2: pad 2 written in 32-channel planes (un-permuted here)
    out = np.empty((B, Ho, Ho, Cc), dtype=np.float32)
    _check(lib, lib.glass_op_blur(device, mode, B, H, Cc, _fp(x), _fp(out)))
    return from_planar32(out, B, Ho, Ho, Cc) if mode == 2 else out


def dblock_down(h, x, w1, wskip, b1, device=0):
    """Fused second half of a D block (conv_down.hip).  h, x [B,R,R,Cin] NHWC; w1 [Cout,Cin,3,3]; wskip [Cout,Cin,1,1]."""
    lib = _lib()
    h, x, w1, wskip, b1 = _f32(h), _f32(x), _f32(w1), _f32(wskip), _f32(b1)
    B, R, _, Cin = h.shape
    Cout = w1.shape[0]
    out = np.full((B, R // 2, R // 2, Cout), np.nan, dtype=np.float32)
    _check(lib, lib.glass_op_dblock_down(device, B, R, Cin, Cout, _fp(h), _fp(x), _fp(w1), _fp(wskip), _fp(b1), _fp(out)))
    return out


def dblock0(y, frgb_w, frgb_b, w0, b0, w1, wskip, b1, impl=0, device=0):
    """The discriminator's whole full-resolution block (conv_d0.hip): y [B,3,R,R] -> [B,R/2,R/2,64].  impl 1: the two-kernel form;
    2: the fused kernel writing chunk-planar (un-permuted here)."""
    lib = _lib()
    y, frgb_w, frgb_b, w0, b0, w1, wskip, b1 = (_f32(a) for a in (y, frgb_w, frgb_b, w0, b0, w1, wskip, b1))
    B, _, R, _ = y.shape
    out = np.full((B, R // 2, R // 2, 64), np.nan, dtype=np.float32)
    _check(lib, lib.glass_op_dblock0(device, B, R, impl, _fp(y), _fp(frgb_w), _fp(frgb_b), _fp(w0), _fp(b0), _fp(w1), _fp(wskip),
                                     _fp(b1), _fp(out)))
    return from_planar8(out, B, R // 2, R // 2, 64) if impl == 2 else out


def fromrgb(y, w, bias, device=0):
    lib = _lib()
    y, w, bias = _f32(y), _f32(w), _f32(bias)
    B, _, R, _ = y.shape
    Cout = w.shape[0]
    out = np.empty((B, R, R, Cout), dtype=np.float32)
    _check(lib, lib.glass_op_fromrgb(device, B, R, Cout, _fp(y), _fp(w), _fp(bias), _fp(out)))
    return out


def mbstd(x, Cpad, batch_size, group=4, device=0):
    lib = _lib()
    x = _f32(x)
    B, hw, Cc = x.shape
    out = np.empty((B, hw, Cpad), dtype=np.float32)
    _check(lib, lib.glass_op_mbstd(device, B, hw, Cc, Cpad, batch_size, group, _fp(x), _fp(out)))
    return out


def resize(y, S, ps, device=0):
    lib = _lib()
    y = _f32(y)
    B, _, R, _ = y.shape
    G = S // ps
    out = np.empty((B * G * G, 3 * ps * ps), dtype=np.float32)
    _check(lib, lib.glass_op_resize(device, B, R, S, ps, _fp(y), _fp(out)))
    return out


def view_patches(y, S, ps, boxes, normalize=0, device=0):
    """The engine's crop-view resize on images [B,3,R,R] in (-1, 1) and boxes int [V,4] = (x0, y0, s, flip); rows (b V + v) G G + g, columns
    as `resize`."""
    lib = _lib()
    y = _f32(y)
    B, _, R, _ = y.shape
    bx = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
    V, G = bx.shape[0], S // ps
    out = np.empty((B * V * G * G, 3 * ps * ps), dtype=np.float32)
    _check(lib, lib.glass_op_view_patches(device, B, R, S, ps, int(normalize), V, bx.ctypes.data_as(ip), _fp(y), _fp(out)))
    return out


def preprocess(y, S, ps, resize_mode=0, normalize=0, device=0):
    """The engine's CLIP preprocessing (glass_config.clip_resize / clip_normalize) on images [B,3,R,R] in (-1, 1); output as `resize`."""
    lib = _lib()
    y = _f32(y)
    B, _, R, _ = y.shape
    G = S // ps
    out = np.empty((B * G * G, 3 * ps * ps), dtype=np.float32)
    _check(lib, lib.glass_op_preprocess(device, B, R, S, ps, int(resize_mode), int(normalize), _fp(y), _fp(out)))
    return out


def layernorm(x, g, b, device=0):
    lib = _lib()
    x, g, b = _f32(x), _f32(g), _f32(b)
    out = np.empty_like(x)
    _check(lib, lib.glass_op_layernorm(device, x.shape[0], x.shape[1], _fp(x), _fp(g), _fp(b), _fp(out)))
    return out


def attention(qkv, n_img, L, heads, causal=False, device=0):
    lib = _lib()
    qkv = _f32(qkv)
    out = np.empty((n_img * L, heads * 64), dtype=np.float32)
    _check(lib, lib.glass_op_attention(device, n_img, L, heads, int(causal), _fp(qkv), _fp(out)))
    return out


def noise(n_mb, hw, layer, mb0, generation, seed, device=0):
    lib = _lib()
    out = np.empty((n_mb, hw), dtype=np.float32)
    _check(lib, lib.glass_op_noise(device, n_mb, hw, layer, mb0, generation, seed, _fp(out)))
    return out


def noise_period(n_mb, hw, layer, mb0, generation, seed, period, device=0):
    """noise() with launch_noise's period: plane m is that of minibatch (mb0 + m) % period (the device search's islands)."""
    lib = _lib()
    out = np.empty((n_mb, hw), dtype=np.float32)
    _check(lib, lib.glass_op_noise_period(device, n_mb, hw, layer, mb0, generation, seed, int(period), _fp(out)))
    return out


def gpt2_sample(logits, temperature, top_k, seed, generation, first_row, step, purpose=0, device=0):
    """The GPT-2 stochastic pick on logits [rows, V] float32 (gpt2.hip, generic path) -> int32 tokens [rows]."""
    lib = _lib()
    lg = _f32(logits)
    rows, V = lg.shape
    out = np.empty(rows, dtype=np.int32)
    _check(lib, lib.glass_op_gpt2_sample(device, rows, V, _fp(lg), float(temperature), int(top_k), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                         int(generation), int(first_row), int(step), int(purpose), out.ctypes.data_as(ip)))
    return out


GPT2_GEMM_FORMS = {"prefill": 0, "decode": 1, "step": 2, "rowblk": 3}


def gpt2_gemm(a, w, bias=None, mode=0, form="step", res=None, ln=None, pst_in=None, want_pst=False, width=None, device=0):
    """A GPT-2 trunk product (gpt2.hip) launched as the engine launches it: out = a[M, :K] @ w[N, K]^T (+ bias), mode 0 plain / 1 GELU-tanh /
    2 `res` + (in place on the device).  `a` may be a view with a row stride > K.  form: "prefill" / "decode" (launch_gemm_f32), "step"
    (launch_gemm_f32_step + its finishing launch), "rowblk" (launch_gemm_f32_rowblk).  ln = (gain, bias): LayerNorm fused on the operand
    from the device's own row statistics ("step": gpt2_finalize_kernel; "rowblk": pst_in, the partials an earlier rowblk call returned).
    Returns a dict: out [M, N], S (the global K split), stats [M, 2] (step form: the fused LayerNorm's, or those a residual product
    leaves), pst [M, N/32, 2] (rowblk with want_pst)."""
    lib = _lib()
    a = np.asarray(a, dtype=np.float32)
    assert a.ndim == 2 and a.strides[1] == 4 and a.strides[0] % 4 == 0
    M, K = a.shape
    lda = a.strides[0] // 4 if M > 1 else K
    abuf = np.zeros((M, lda), dtype=np.float32)
    abuf[:, :K] = a
    if lda > K:                                     # what lies between the rows is not the product's business
        abuf[:, K:] = np.nan
    w = _f32(w)
    N = w.shape[0]
    assert w.shape == (N, K)
    f = GPT2_GEMM_FORMS[form]
    out = np.empty((M, N), dtype=np.float32)
    if mode == 2:
        out[...] = res
    bias_a, bias_p = _opt(bias)
    g_a, g_p = _opt(None if ln is None else ln[0])
    b_a, b_p = _opt(None if ln is None else ln[1])
    pi_a, pi_p = _opt(pst_in)
    np_in = 0 if pst_in is None else int(pi_a.shape[1])
    stats = np.full((M, 2), np.nan, dtype=np.float32)
    pst = np.full((M, max(N // 32, 1), 2), np.nan, dtype=np.float32) if want_pst else None
    S = C.c_int32(0)
    _check(lib, lib.glass_op_gpt2_gemm(device, f, M, N, K, lda, int(mode), int(width or min(N, K)), _fp(abuf), _fp(w), bias_p, g_p, b_p, pi_p,
                                       np_in, _fp(out), _fp(stats), None if pst is None else _fp(pst), C.byref(S)))
    return dict(out=out, S=int(S.value), stats=stats, pst=pst)


def gpt2_attention(qkv, kc, vc, past, heads, form="general", bias=None, device=0):
    """One GPT-2 attention launch (gpt2.hip) over caches kc / vc [P, Tmax, D].  form "general": gpt2_attention_kernel with the host's
    past; "general_dev": the same kernel with `past` in device memory (the graph-replay form); "step": gpt2_attention_step_kernel.
    qkv: [P * nd, 3 D] finished values, or for "step" [S, P, 3 D] split-K slices (summed by the kernel, + bias [3 D]).
    Returns (out [P * nd, D], kc, vc) — the caches after the call."""
    lib = _lib()
    kc, vc = np.array(kc, dtype=np.float32, order="C"), np.array(vc, dtype=np.float32, order="C")
    P, Tmax, D = kc.shape
    assert vc.shape == kc.shape and D == heads * 64
    qkv = _f32(qkv)
    f = {"general": 0, "general_dev": 1, "step": 2}[form]
    if qkv.ndim == 3:
        S, nd = qkv.shape[0], 1
        assert f == 2 and qkv.shape[1:] == (P, 3 * D)
    else:
        S, nd = 0, qkv.shape[0] // P
        assert qkv.shape == (P * nd, 3 * D)
    out = np.empty((P * nd, D), dtype=np.float32)
    bias_a, bias_p = _opt(bias)
    _check(lib, lib.glass_op_gpt2_attention(device, f, P, nd, int(past), Tmax, heads, S, _fp(qkv), bias_p, _fp(kc), _fp(vc), _fp(out)))
    return out, kc, vc


def gpt2_head(x, wte, lng, lnb, tail=False, wpe=None, past=0, step=0, device=0):
    """The vocabulary head of a single-token step (gpt2.hip): row statistics by gpt2_finalize_kernel, then launch_gpt2_head with the arg-max pick (tail=False:
    returns logits [M, V], pair_val / pair_idx [M, ceil(V/32)], token [M], stats [M, 2]) or with the arg-max + embed / advance tail at the state
    {past, step, 0} (tail=True: token, stats, x_next [M, K], stats_next [M, 2], state [3])."""
    lib = _lib()
    x, wte, lng, lnb = _f32(x), _f32(wte), _f32(lng), _f32(lnb)
    M, K = x.shape
    V = wte.shape[0]
    NB = (V + 31) // 32
    token = np.full(M, -1, dtype=np.int32)
    stats = np.full((M, 2), np.nan, dtype=np.float32)
    if not tail:
        logits = np.empty((M, V), dtype=np.float32)
        pv = np.empty((M, NB), dtype=np.float32)
        pi = np.empty((M, NB), dtype=np.int32)
        _check(lib, lib.glass_op_gpt2_head(device, M, V, K, 0, _fp(x), _fp(wte), _fp(lng), _fp(lnb), None, 0, 0, 0, _fp(logits), _fp(pv),
                                           pi.ctypes.data_as(ip), token.ctypes.data_as(ip), _fp(stats), None, None, None))
        return dict(logits=logits, pair_val=pv, pair_idx=pi, token=token, stats=stats)
    wpe = _f32(wpe)
    x_next = np.full((M, K), np.nan, dtype=np.float32)
    stats_next = np.full((M, 2), np.nan, dtype=np.float32)
    state = np.full(3, -1, dtype=np.int32)
    _check(lib, lib.glass_op_gpt2_head(device, M, V, K, 1, _fp(x), _fp(wte), _fp(lng), _fp(lnb), _fp(wpe), wpe.shape[0], int(past), int(step),
                                       None, None, None, token.ctypes.data_as(ip), _fp(stats), _fp(x_next), _fp(stats_next),
                                       state.ctypes.data_as(ip)))
    return dict(token=token, stats=stats, x_next=x_next, stats_next=stats_next, state=state)


def gpt2_embed_step(token, wte, wpe, past, step, device=0):
    """launch_gpt2_embed_step with statistics at the state {past, step}: (x [M, K] = wte[token] + wpe[past], stats [M, 2])."""
    lib = _lib()
    wte, wpe = _f32(wte), _f32(wpe)
    tok = np.ascontiguousarray(token, dtype=np.int32)
    M, (V, K) = tok.shape[0], wte.shape
    x = np.full((M, K), np.nan, dtype=np.float32)
    stats = np.full((M, 2), np.nan, dtype=np.float32)
    _check(lib, lib.glass_op_gpt2_embed_step(device, M, V, K, tok.ctypes.data_as(ip), _fp(wte), _fp(wpe), wpe.shape[0], int(past), int(step),
                                             _fp(x), _fp(stats)))
    return x, stats


def bg_cond(x, et, zd, device=0):
    """bg_cond_kernel: population rows x [P, zd + nc] = [z | class bits], et = E^T [nc, zd] -> cond [P, 2 zd] = [clip(z, -2, 2) | softmax @ E^T]."""
    lib = _lib()
    x, et = _f32(x), _f32(et)
    P, L = x.shape
    nc = et.shape[0]
    assert et.shape == (nc, zd) and L >= zd + nc
    cond = np.empty((P, 2 * zd), dtype=np.float32)
    _check(lib, lib.glass_op_bg_cond(device, P, L, zd, nc, _fp(x), _fp(et), _fp(cond)))
    return cond


def bg_bn_tables(cond, wt, bias, inv_std, mean, prebias, device=0):
    """The three launches of glass_biggan_prepare (dense + bg_bn_tables_kernel + bg_to_half_kernel): cond [P, cd], wt [cd, 2C] (gain | offset
    columns), bias [2C], inv_std / mean / prebias [C] -> (tab [P, 2C] = [A | S] float32, tab16: its fp16 copy as float32 values)."""
    lib = _lib()
    cond, wt, bias, inv_std, mean, prebias = (_f32(a) for a in (cond, wt, bias, inv_std, mean, prebias))
    P, cd = cond.shape
    Cc = inv_std.shape[0]
    assert wt.shape == (cd, 2 * Cc) and bias.shape == (2 * Cc,) and mean.shape == (Cc,) and prebias.shape == (Cc,)
    tab = np.empty((P, 2 * Cc), dtype=np.float32)
    tab16 = np.empty((P, 2 * Cc), dtype=np.float32)
    _check(lib, lib.glass_op_bg_bn_tables(device, P, cd, Cc, _fp(cond), _fp(wt), _fp(bias), _fp(inv_std), _fp(mean), _fp(prebias), _fp(tab),
                                          _fp(tab16)))
    return tab, tab16


def bg_attn_split(T, c8, c2, device=0):
    """T [B,H,W,2 c8 + c2] (theta | phi | g) -> (theta [B,HW,c8], phi [B,HW/4,c8], gT [B,c2,HW/4], kernel name): the split + 2x2
    max-pool + transpose of the self-attention block; the name says which of the launcher's two kernels ran."""
    lib = _lib()
    T = _f32(T)
    B, H, W, CT = T.shape
    assert CT == 2 * c8 + c2
    hw = H * W
    theta = np.empty((B, hw, c8), dtype=np.float32)
    phi = np.empty((B, hw // 4, c8), dtype=np.float32)
    gT = np.empty((B, c2, hw // 4), dtype=np.float32)
    vec = C.c_int32(-1)
    _check(lib, lib.glass_op_bg_attn_split(device, B, H, W, c8, c2, _fp(T), _fp(theta), _fp(phi), _fp(gT), C.byref(vec)))
    return theta, phi, gT, "bg_attn_split_vec_kernel" if vec.value == 1 else "bg_attn_split_kernel"


def bg_softmax(S, device=0):
    """Row softmax S [rows, n] float32 -> [rows, n] (the kernel's fp16 values)."""
    lib = _lib()
    S = _f32(S)
    rows, n = S.shape
    out = np.empty((rows, n), dtype=np.float32)
    _check(lib, lib.glass_op_bg_softmax(device, rows, n, _fp(S), _fp(out)))
    return out


def bg_rgb_tanh(x, device=0):
    """x [B, hw, C] (rounded to fp16) -> [B, 3, hw] = tanh of channels 0..2, planar float32."""
    lib = _lib()
    x = _f32(x)
    B, hw, Cc = x.shape
    y = np.empty((B, 3, hw), dtype=np.float32)
    _check(lib, lib.glass_op_bg_rgb_tanh(device, B, hw, Cc, _fp(x), _fp(y)))
    return y


def bg_to_half(x, device=0):
    """bg_to_half_kernel on a flat float32 array of any length -> its fp16 values (as float32)."""
    lib = _lib()
    x = _f32(x).reshape(-1)
    out = np.empty(x.shape, dtype=np.float32)
    _check(lib, lib.glass_op_bg_to_half(device, x.shape[0], _fp(x), _fp(out)))
    return out


def bg_tail(h, x0, w3, b3, bn_a, bn_s, rgb_w, rgb_b, device=0):
    """BigGAN-deep's fused last stage (bg_tail.hip): h [B,R,R,mid] (= relu(bn_3(conv_2))), x0 [B,R/2,R/2,128] (the block input), w3 [128,mid],
    b3 [128], the final bn's folded A / S [128], rgb_w [3,128,3,3], rgb_b [3] -> tanh(conv_to_rgb(relu(bn(conv_3(h) + up(x0))))) [B,3,R,R]."""
    lib = _lib()
    h, x0, w3, b3, bn_a, bn_s, rgb_w, rgb_b = (_f32(a) for a in (h, x0, w3, b3, bn_a, bn_s, rgb_w, rgb_b))
    B, R, _, mid = h.shape
    assert w3.shape[0] == 128 and w3.size == 128 * mid and rgb_w.shape == (3, 128, 3, 3) and b3.shape == bn_a.shape == bn_s.shape == (128,)
    assert x0.shape == (B, R // 2, R // 2, 128) and rgb_b.shape == (3,)
    y = np.empty((B, 3, R, R), dtype=np.float32)
    _check(lib, lib.glass_op_bg_tail(device, B, R, mid, _fp(h), _fp(x0), _fp(w3), _fp(b3), _fp(bn_a), _fp(bn_s), _fp(rgb_w), _fp(rgb_b), _fp(y)))
    return y


# ---- CLIP's ResNet towers (glass_op_rn_*): each piece as the tower's walker launches it; BatchNorm as fp32 scale bn_a / shift bn_s ----
def rn_avgpool(x, device=0):
    """AvgPool2d(2) of x [B,H,W,C] -> [B,H/2,W/2,C]."""
    lib = _lib()
    x = _f32(x)
    B, H, W, Cc = x.shape
    out = np.empty((B, H // 2, W // 2, Cc), np.float32)
    _check(lib, lib.glass_op_rn_avgpool(device, B, H, W, Cc, _fp(x), _fp(out)))
    return out


def rn_stem_conv1(img, w, bn_a, bn_s, device=0):
    """img [B,3,S,S], w [C1,3,3,3] -> relu(bn(conv 3x3 stride 2 pad 1)) [B,S/2,S/2,C1], read through the 32-pixel patch operand."""
    lib = _lib()
    img, w, bn_a, bn_s = _f32(img), _f32(w), _f32(bn_a), _f32(bn_s)
    B, S, C1 = img.shape[0], img.shape[2], w.shape[0]
    out = np.empty((B, S // 2, S // 2, C1), np.float32)
    _check(lib, lib.glass_op_rn_stem_conv1(device, B, S, C1, _fp(img), _fp(w), _fp(bn_a), _fp(bn_s), _fp(out)))
    return out


def rn_conv_bn(x, w, bn_a, bn_s, res=None, relu=True, form=0, device=0):
    """act(conv(x, w) * bn_a + bn_s (+ res)), x [B,H,W,Cin], w [Cout,Cin,KS,KS] (KS 1 or 3, stride 1, pad KS // 2).  form 0: gemm_tiled as the
    bottlenecks run it; form 1: the stem's 3 x 3 kernel."""
    lib = _lib()
    x, w, bn_a, bn_s = _f32(x), _f32(w), _f32(bn_a), _f32(bn_s)
    B, H, W, Cin = x.shape
    Cout, KS = w.shape[0], w.shape[2]
    r, rp = _opt(res)
    out = np.empty((B, H, W, Cout), np.float32)
    _check(lib, lib.glass_op_rn_conv_bn(device, int(form), B, H, W, Cin, Cout, KS, int(bool(relu)), _fp(x), _fp(w), _fp(bn_a), _fp(bn_s), rp,
                                        _fp(out)))
    return out


def rn_tokens(x, pos, device=0):
    """x [B,HW,C], pos [HW+1,C] -> the attention pool's tokens [B,HW+1,C]."""
    lib = _lib()
    x, pos = _f32(x), _f32(pos)
    B, HW, Cc = x.shape
    out = np.empty((B, HW + 1, Cc), np.float32)
    _check(lib, lib.glass_op_rn_tokens(device, B, HW, Cc, _fp(x), _fp(pos), _fp(out)))
    return out


# ---- the small fp32 kernels around StyleGAN2 and the CLIP towers (glass_op_mapping ... glass_op_rn_token0_rows) ----
# ---- perceptual objective (csrc/lpips.hip) ----
def lpips_input(y, S, device=0):
    """y [B,3,R,R] fp32 -> [B,S,S,4]: box mean to S, (v - shift_c) / scale_c, rounded to fp16; channel 3 = 0."""
    lib = _lib()
    y = _f32(y)
    B, _, R, _ = y.shape
    out = np.empty((B, S, S, 4), dtype=np.float32)
    _check(lib, lib.glass_op_lpips_input(device, B, R, S, _fp(y), _fp(out)))
    return out


def vgg_conv1(x, w, bias, device=0):
    """x [B,S,S,4] (lpips_input's layout), w [64,3,3,3], bias [64] -> relu(conv3x3 pad 1 + bias) [B,S,S,64]."""
    lib = _lib()
    x, w, bias = _f32(x), _f32(w), _f32(bias)
    B, S = x.shape[0], x.shape[1]
    out = np.empty((B, S, S, 64), dtype=np.float32)
    _check(lib, lib.glass_op_vgg_conv1(device, B, S, _fp(x), _fp(w), _fp(bias), _fp(out)))
    return out


def maxpool2(x, device=0):
    """MaxPool2d(2) of x [B,H,W,C] -> [B,H/2,W/2,C]."""
    lib = _lib()
    x = _f32(x)
    B, H, W, Cc = x.shape
    out = np.empty((B, H // 2, W // 2, Cc), dtype=np.float32)
    _check(lib, lib.glass_op_maxpool2(device, B, H, W, Cc, _fp(x), _fp(out)))
    return out


def lpips_head(x0, x1, lin, device=0):
    """x0 [n,HW,C], x1 [n,HW,C] or [1,HW,C] (one map for all), lin [C] -> [n]: one slice's term of the distance."""
    lib = _lib()
    x0, x1, lin = _f32(x0), _f32(x1), _f32(lin)
    n, HW, Cc = x0.shape
    shared = int(x1.shape[0] == 1 and n > 1)
    out = np.empty((n,), dtype=np.float32)
    _check(lib, lib.glass_op_lpips_head(device, n, HW, Cc, shared, _fp(x0), _fp(x1), _fp(lin), _fp(out)))
    return out


MAP_FUSED, MAP_PIXELNORM, MAP_SPLITK, MAP_DENSE = 1, 2, 4, 8
MAPPING_PATHS = {"auto": 0, "layers": 1, "fused": 2}


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ip)


def _strided(a, ld, fill=np.nan):
    """[rows, n] -> a [rows, ld] float32 buffer with `fill` between the rows: a read outside a row shows."""
    a = np.asarray(a, dtype=np.float32)
    buf = np.full((a.shape[0], ld), fill, dtype=np.float32)
    buf[:, :a.shape[1]] = a
    return buf


def mapping(z, wt, b, path="auto", device=0):
    """The mapping network through the launcher run_mapping calls: z [P, L], wt [n_layers, L, L] (each [k, n], coefficient folded), b
    [n_layers, L] -> (w [P, L], the set of kernels that ran).  path "auto": as the engine decides; "layers": pixel norm + one dense launch
    per layer; "fused": mapping_fused_kernel or an error."""
    lib = _lib()
    z, wt, b = _f32(z), _f32(wt), _f32(b)
    P, L = z.shape
    n = wt.shape[0]
    assert wt.shape == (n, L, L) and b.shape == (n, L)
    out = np.empty((P, L), dtype=np.float32)
    ran = C.c_int32(0)
    _check(lib, lib.glass_op_mapping(device, P, L, n, _fp(z), _fp(wt), _fp(b), MAPPING_PATHS[path], _fp(out), C.byref(ran)))
    names = {MAP_FUSED: "mapping_fused_kernel", MAP_PIXELNORM: "pixelnorm_kernel", MAP_SPLITK: "dense_splitk_kernel", MAP_DENSE: "dense_kernel"}
    return out, {v for k, v in names.items() if ran.value & k}


def pixelnorm(z, device=0):
    lib = _lib()
    z = _f32(z)
    out = np.empty_like(z)
    _check(lib, lib.glass_op_pixelnorm(device, z.shape[0], z.shape[1], _fp(z), _fp(out)))
    return out


def dense_splitk(x, wt, bias=None, mode=0, ldx=None, ldo=None, device=0):
    """dense_splitk_kernel on x [P, K] stored with row stride ldx (NaN between the rows) -> the whole output table [P, ldo]; the columns
    past N come back as the NaN they were uploaded with."""
    lib = _lib()
    wt = _f32(wt)
    P, K = np.shape(x)
    N = wt.shape[1]
    ldx, ldo = ldx or K, ldo or N
    xb = _strided(x, ldx)
    out = np.full((P, ldo), np.nan, dtype=np.float32)
    bb, bp = _opt(bias)
    _check(lib, lib.glass_op_dense_splitk(device, P, K, N, ldx, ldo, mode, _fp(xb), _fp(wt), bp, _fp(out)))
    return out


def dense_ex(x, wt, bias=None, in_sq=False, mode=0, eps_row=None, ldx=None, out=None, col0=0, device=0):
    """dense_kernel with the strides the style path uses: x [P, K] stored with row stride ldx (NaN between the rows); the result goes to
    columns col0 .. col0 + N of the table `out` [P, ldo] (default: a NaN table of width N), which is returned whole.  eps_row [P, stride]:
    mode 2 reads column 0."""
    lib = _lib()
    wt = _f32(wt)
    P, K = np.shape(x)
    N = wt.shape[1]
    xb = _strided(x, ldx or K)
    out = np.full((P, N), np.nan, dtype=np.float32) if out is None else np.array(out, dtype=np.float32, order="C")
    ldo = out.shape[1]
    assert col0 + N <= ldo
    bb, bp = _opt(bias)
    e, ep = _opt(None if eps_row is None else np.reshape(eps_row, (P, -1)))
    buf = np.concatenate([out.reshape(-1), np.full(col0, np.nan, np.float32)])
    win = buf[col0:]                                    # the launch's `out` pointer is column col0 of row 0: [P, ldo] floats from there on
    _check(lib, lib.glass_op_dense_ex(device, P, K, N, xb.shape[1], ldo, _fp(xb), _fp(wt), bp, int(in_sq), mode, ep,
                                      0 if e is None else e.shape[1], win.ctypes.data_as(fp)))
    return buf[:out.size].reshape(out.shape)


def dense_multi(x, problems, eps_rows, ldo, device=0):
    """The demodulation launch (dense_multi_kernel, in_sq 1, mode 2): x [P, ldx] the shared style table, problems a list of (x_off, wt [K, N],
    out_off, eps_idx), eps_rows [P, n_style] -> the output table [P, ldo] (NaN where no problem writes)."""
    lib = _lib()
    x, eps_rows = _f32(x), _f32(eps_rows)
    P, ldx = x.shape
    wts = [_f32(q[1]) for q in problems]
    K, Kp = _i32([w.shape[0] for w in wts]); N, Np = _i32([w.shape[1] for w in wts])
    xo, xop = _i32([q[0] for q in problems]); oo, oop = _i32([q[2] for q in problems]); ei, eip = _i32([q[3] for q in problems])
    wt = np.concatenate([w.reshape(-1) for w in wts])
    out = np.full((P, ldo), np.nan, dtype=np.float32)
    _check(lib, lib.glass_op_dense_multi(device, len(problems), P, ldx, ldo, eps_rows.shape[1], Kp, Np, xop, oop, eip, _fp(x), _fp(wt),
                                         _fp(eps_rows), _fp(out)))
    return out


def style_norm(s, segments, device=0):
    """style_norm_kernel (eps 1e-8) over the (offset, length) segments of each row of s [P, ld] -> (s normalised, smax [P, n], eps_row [P, n])."""
    lib = _lib()
    s = np.array(s, dtype=np.float32, order="C")
    P, ld = s.shape
    off, offp = _i32([q[0] for q in segments]); ln, lnp = _i32([q[1] for q in segments])
    n = len(segments)
    smax, eps_row = np.empty((P, n), np.float32), np.empty((P, n), np.float32)
    _check(lib, lib.glass_op_style_norm(device, P, ld, n, offp, lnp, _fp(s), _fp(smax), _fp(eps_row)))
    return s, smax, eps_row


def d_head(dfin, w0, b0, w1, b1, device=0):
    """D's dense head through the launchers run_d_head calls: dfin [P, 16 CL], w0 [CL, 16 CL] (both rounded to fp16 on upload), b0 [CL],
    w1 [CL], b1 [1] -> (dis [P], "split" | "whole": the form that ran)."""
    lib = _lib()
    dfin, w0, b0, w1, b1 = (_f32(a) for a in (dfin, w0, b0, w1, b1))
    P, CL = dfin.shape[0], w0.shape[0]
    assert dfin.shape == (P, 16 * CL) and w0.shape == (CL, 16 * CL) and b0.shape == (CL,) and w1.shape == (CL,) and b1.shape == (1,)
    dis = np.empty(P, dtype=np.float32)
    split = C.c_int32(-1)
    _check(lib, lib.glass_op_d_head(device, P, CL, _fp(dfin), _fp(w0), _fp(b0), _fp(w1), _fp(b1), _fp(dis), C.byref(split)))
    return dis, "split" if split.value == 1 else "whole"


def finalize_image(y, device=0):
    lib = _lib()
    y = _f32(y)
    img = np.empty_like(y)
    _check(lib, lib.glass_op_finalize_image(device, y.size, _fp(y), _fp(img)))
    return img


def embed_lnpre(patch_emb, cls, pos, g, b, device=0):
    """patch_emb [P, T - 1, D], cls [D], pos [T, D], ln_pre g / b [D] -> tokens [P, T, D]."""
    lib = _lib()
    patch_emb, cls, pos, g, b = (_f32(a) for a in (patch_emb, cls, pos, g, b))
    P, T1, D = patch_emb.shape
    assert pos.shape == (T1 + 1, D)
    x = np.empty((P, T1 + 1, D), dtype=np.float32)
    _check(lib, lib.glass_op_embed_lnpre(device, P, T1 + 1, D, _fp(patch_emb), _fp(cls), _fp(pos), _fp(g), _fp(b), _fp(x)))
    return x


def embed_text(tokens, tok_emb, pos, device=0):
    """tokens int [n, ctx], tok_emb [V, D], pos [ctx, D] -> [n * ctx, D]."""
    lib = _lib()
    tok, tokp = _i32(tokens)
    tok_emb, pos = _f32(tok_emb), _f32(pos)
    n, ctx = tok.shape
    V, D = tok_emb.shape
    x = np.empty((n * ctx, D), dtype=np.float32)
    _check(lib, lib.glass_op_embed_text(device, n, ctx, D, V, tokp, _fp(tok_emb), _fp(pos), _fp(x)))
    return x


def layernorm_ex(x, g, b, row_stride=None, half_out=False, device=0):
    """layernorm_kernel on the rows of x [M, D] stored row_stride apart (NaN between them); half_out: the fp16 output (as float32 values)."""
    lib = _lib()
    g, b = _f32(g), _f32(b)
    M, D = np.shape(x)
    xb = _strided(x, row_stride or D)
    out = np.empty((M, D), dtype=np.float32)
    _check(lib, lib.glass_op_layernorm_ex(device, M, D, xb.shape[1], int(half_out), _fp(xb), _fp(g), _fp(b), _fp(out)))
    return out


def layernorm_rows(x, rows, g, b, device=0):
    lib = _lib()
    x, g, b = _f32(x), _f32(g), _f32(b)
    r, rp = _i32(rows)
    out = np.empty((r.shape[0], x.shape[1]), dtype=np.float32)
    _check(lib, lib.glass_op_layernorm_rows(device, x.shape[0], r.shape[0], x.shape[1], _fp(x), rp, _fp(g), _fp(b), _fp(out)))
    return out


def cosine(feat, target, device=0):
    lib = _lib()
    feat, target = _f32(feat), _f32(target)
    P, D = feat.shape
    sim = np.empty(P, dtype=np.float32)
    _check(lib, lib.glass_op_cosine(device, P, D, _fp(feat), _fp(target), _fp(sim)))
    return sim


def cosine_views(feat, target, device=0):
    """feat [P, V, D] -> (view_sim [P, V], sim [P])."""
    lib = _lib()
    feat, target = _f32(feat), _f32(target)
    P, V, D = feat.shape
    vs, sim = np.empty((P, V), np.float32), np.empty(P, np.float32)
    _check(lib, lib.glass_op_cosine_views(device, P, V, D, _fp(feat), _fp(target), _fp(vs), _fp(sim)))
    return vs, sim


def cosine_set(feat, targets, weights, device=0):
    """feat [P, V, D], targets [T, D], weights [T] -> (view_sim [P, V], set_sim [P, T], sim [P]): cosine_set_kernel (prompt sets)."""
    lib = _lib()
    feat, targets, weights = _f32(feat), _f32(targets), _f32(weights)
    P, V, D = feat.shape
    T = targets.shape[0]
    vs, ss, sim = np.empty((P, V), np.float32), np.empty((P, T), np.float32), np.empty(P, np.float32)
    _check(lib, lib.glass_op_cosine_set(device, P, V, T, D, _fp(feat), _fp(targets), _fp(weights), _fp(vs), _fp(ss), _fp(sim)))
    return vs, ss, sim


def cosine_set_islands(feat, targets, weights, pop, row0=0, device=0):
    """cosine_set with an island table (include/glass.h "Device search: islands", own prompts): weights [islands, T]; row p of feat [P, V, D]
    is search row row0 + p and takes the weights of island (row0 + p) // pop."""
    lib = _lib()
    feat, targets, weights = _f32(feat), _f32(targets), _f32(weights)
    P, V, D = feat.shape
    T = targets.shape[0]
    vs, ss, sim = np.empty((P, V), np.float32), np.empty((P, T), np.float32), np.empty(P, np.float32)
    _check(lib, lib.glass_op_cosine_set_islands(device, P, V, T, D, _fp(feat), _fp(targets), _fp(weights), weights.shape[0], int(pop), int(row0),
                                                _fp(vs), _fp(ss), _fp(sim)))
    return vs, ss, sim


def assemble_F_set(set_sim, weights, dis=None, lp=None, device=0):
    """set_sim [P, K], weights [K], dis / lp [P] or None -> F [P, K + (dis is not None) + (lp is not None)]: the pareto layout."""
    lib = _lib()
    set_sim, weights = _f32(set_sim), _f32(weights)
    P, K = set_sim.shape
    d, dp = _opt(dis)
    l, lpp = _opt(lp)
    Fv = np.empty((P, K + (dis is not None) + (lp is not None)), dtype=np.float32)
    _check(lib, lib.glass_op_assemble_F_set(device, P, K, _fp(set_sim), _fp(weights), dp, lpp, _fp(Fv)))
    return Fv


def cosine_set_dir(feat, targets, weights, src, streamed=False, device=0):
    """feat [P, V, D], targets [T, D], weights [T], src [V, D] (unit rows) -> (view_sim [P, V], set_sim [P, T], sim [P]): cosine_set_kernel's directional form
    (image editing), the cosine of f / |f| - src[v] with every entry.  streamed: the form that reads the set from memory at any shape."""
    lib = _lib()
    feat, targets, weights, src = _f32(feat), _f32(targets), _f32(weights), _f32(src)
    P, V, D = feat.shape
    T = targets.shape[0]
    if targets.shape != (T, D) or weights.shape != (T,) or src.shape != (V, D):
        raise ValueError("cosine_set_dir: targets [T, %d], weights [T] and src [%d, %d] expected, got %r, %r, %r"
                         % (D, V, D, targets.shape, weights.shape, src.shape))
    vs, ss, sim = np.empty((P, V), np.float32), np.empty((P, T), np.float32), np.empty(P, np.float32)
    _check(lib, lib.glass_op_cosine_set_dir(device, P, V, T, D, _fp(feat), _fp(targets), _fp(weights), _fp(src), int(bool(streamed)), _fp(vs),
                                            _fp(ss), _fp(sim)))
    return vs, ss, sim


def latent_anchor(w, a, device=0):
    """w [P, n_lat, L], or [P, L] (one row for every layer), a [n_lat, L] -> d [P] = mean (w - a)^2: latent_anchor_kernel (image editing)."""
    lib = _lib()
    w, a = _f32(w), _f32(a)
    n_lat, L = a.shape
    if w.shape[1:] not in ((n_lat, L), (L,)):
        raise ValueError("latent_anchor: w must be [P, %d, %d] or [P, %d], got %r" % (n_lat, L, L, w.shape))
    d = np.empty(w.shape[0], np.float32)
    _check(lib, lib.glass_op_latent_anchor(device, w.shape[0], n_lat, L, int(w.ndim == 3), _fp(w), _fp(a), _fp(d)))
    return d


def dlatent_subspace(c, layer_group, basis, base, device=0):
    """c [P, G, K] coefficients, layer_group int [n_lat] (-1: frozen), basis [K, L], base [n_lat, L] -> dlatents [P, n_lat, L]:
    dlatent_subspace_kernel (latent space sub, include/glass.h).  The rule's refusals come back as RuntimeError with its words."""
    lib = _lib()
    c, basis, base = _f32(c), _f32(basis), _f32(base)
    lg = np.ascontiguousarray(layer_group, dtype=np.int32)
    if c.ndim != 3 or basis.ndim != 2 or base.ndim != 2 or lg.ndim != 1:
        raise ValueError("dlatent_subspace: c [P, G, K], layer_group [n_lat], basis [K, L] and base [n_lat, L] expected, got %r, %r, %r, %r"
                         % (c.shape, lg.shape, basis.shape, base.shape))
    P, G, K = c.shape
    n_lat, L = base.shape
    if basis.shape != (K, L) or lg.shape != (n_lat,):
        raise ValueError("dlatent_subspace: basis must be [%d, %d] and layer_group [%d], got %r and %r" % (K, L, n_lat, basis.shape, lg.shape))
    out = np.empty((P, n_lat, L), np.float32)
    _check(lib, lib.glass_op_dlatent_subspace(device, _fp(c), P, G, K, lg.ctypes.data_as(ip), n_lat, L, _fp(basis), _fp(base), _fp(out)))
    return out


def assemble_F(sim, dis=None, device=0):
    lib = _lib()
    sim = _f32(sim)
    d, dp = _opt(dis)
    n_obj = 1 if dis is None else 2
    Fv = np.empty((sim.shape[0], n_obj), dtype=np.float32)
    _check(lib, lib.glass_op_assemble_F(device, sim.shape[0], n_obj, _fp(sim), dp, _fp(Fv)))
    return Fv


def image_patches(img, ps, ld, sentinel=-7.0, device=0):
    """img [n, 3, S, S] -> the patch operand [n (S / ps)^2, ld] as fp16 values; the columns the kernel does not write hold `sentinel`."""
    lib = _lib()
    img = _f32(img)
    n, _, S, _ = img.shape
    G = S // ps
    out = np.empty((n * G * G, ld), dtype=np.float32)
    _check(lib, lib.glass_op_image_patches(device, n, S, ps, ld, _fp(img), float(sentinel), _fp(out)))
    return out


def rn_token0_rows(att, device=0):
    """att [B, T, C] (rounded to fp16) -> [B, C] float32 = att[:, 0, :]."""
    lib = _lib()
    att = _f32(att)
    B, T, Cc = att.shape
    out = np.empty((B, Cc), dtype=np.float32)
    _check(lib, lib.glass_op_rn_token0_rows(device, B, T, Cc, _fp(att), _fp(out)))
    return out


def mfma_probe(a, b, device=0):
    lib = _lib()
    a, b = _f32(a), _f32(b)
    d = np.empty((32, 32), dtype=np.float32)
    _check(lib, lib.glass_op_mfma_probe(device, _fp(a), _fp(b), _fp(d)))
    return d


def host_pack_conv(w, up=False):
    """finalize()'s weight repacking, host only: returns [KS*KS][Neff][Cin] float32 (fp16-rounded)."""
    lib = _lib()
    w = _f32(w)
    Cout, Cin, KS, _ = w.shape
    out = np.empty((KS * KS, (4 if up else 1) * Cout, Cin), dtype=np.float32)
    _check(lib, lib.glass_host_pack_conv(_fp(w), Cout, Cin, KS, int(up), _fp(out)))
    return out


RESIZE_MAX_TAPS = 32      # GLASS_RESIZE_MAX_TAPS (csrc/kernels.h): taps per output pixel and axis


def host_resize_taps(R, S, mode, max_taps=RESIZE_MAX_TAPS):
    """finalize()'s tap table of one axis of the antialiased resize R -> S (mode 1 bilinear, 2 bicubic), host only:
    (start int32 [S], count int32 [S], taps float32 [S, max_taps])."""
    lib = _lib()
    start, count = np.empty(S, np.int32), np.empty(S, np.int32)
    taps = np.empty((S, max_taps), np.float32)
    _check(lib, lib.glass_host_resize_taps(R, S, int(mode), start.ctypes.data_as(ip), count.ctypes.data_as(ip), _fp(taps), max_taps))
    return start, count, taps


def host_gpt2_step_plan(P, D, V, n_layer, Tmax, sample=False, n_cu=256):
    """The launches of one GPT-2 token step as the engine's host code makes them, host only: a list of (kernel name, grid (x, y, z),
    block (x, y, z)) in launch order.  n_cu: the compute units the step products' grids are weighed against."""
    lib = _lib()
    buf = C.create_string_buffer(1 << 16)
    _check(lib, lib.glass_host_gpt2_step_plan(P, D, V, n_layer, Tmax, int(bool(sample)), n_cu, buf, len(buf)))
    plan = []
    for line in buf.value.decode().splitlines():
        name, grid, block = line.rsplit(" ", 2)
        plan.append((name, tuple(int(v) for v in grid.split("=")[1].split(",")), tuple(int(v) for v in block.split("=")[1].split(","))))
    return plan


def host_gpt2_gemm_choice(M, N, K, ln=False, width=None, n_cu=256):
    """choose_gemm_f32_step's answer for a [M, K] x [N, K]^T step product, host only: (S, NK) — the global K split (0: refused) and the K parts
    per workgroup — with the split-K scratch gpt2_gemm gives it (width: as there) on a device of n_cu compute units."""
    lib = _lib()
    S, NK = C.c_int32(-1), C.c_int32(-1)
    _check(lib, lib.glass_host_gpt2_gemm_choice(M, N, K, K, int(bool(ln)), int(width or min(N, K)), n_cu, C.byref(S), C.byref(NK)))
    return S.value, NK.value


# ---- device search (csrc/search.hip; include/glass.h "Device search") ------------------------------------------------------------
def ga_vary(X, rank, cd, xl, xu, eta_c=3.0, eta_m=3.0, prob_m=0.5, seed=1, generation=1, row0=0, rows=None, device=0):
    """Offspring rows [row0, row0 + rows) of the population X float32 [pop, n_var] with rank int32 [pop] and cd float64 [pop]."""
    lib = _lib()
    X = _f32(X)
    pop, nv = X.shape
    rows = pop - row0 if rows is None else rows
    rank = np.ascontiguousarray(rank, dtype=np.int32)
    cd = np.ascontiguousarray(cd, dtype=np.float64)
    out = np.empty((rows, nv), dtype=np.float32)
    _check(lib, lib.glass_op_ga_vary(device, pop, nv, _fp(X), rank.ctypes.data_as(ip), cd.ctypes.data_as(dp),
                                     float(xl), float(xu), float(eta_c), float(eta_m), float(prob_m), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                     int(generation), int(row0), int(rows), _fp(out)))
    return out


def ga_vary_mixed(X, n_real, rank, cd, xl, xu, eta_c=3.0, eta_m=3.0, prob_m=0.5, prob_x=0.2, prob_flip=0.01, seed=1, generation=1, row0=0,
                  rows=None, device=0):
    """Offspring rows [row0, row0 + rows) of the mixed population X float32 [pop, n_real + n_bits] (bit columns 0.0 / 1.0)."""
    lib = _lib()
    X = _f32(X)
    pop, nv = X.shape
    rows = pop - row0 if rows is None else rows
    rank = np.ascontiguousarray(rank, dtype=np.int32)
    cd = np.ascontiguousarray(cd, dtype=np.float64)
    out = np.empty((rows, nv), dtype=np.float32)
    _check(lib, lib.glass_op_ga_vary_mixed(device, pop, int(n_real), nv - int(n_real), _fp(X), rank.ctypes.data_as(ip), cd.ctypes.data_as(dp),
                                           float(xl), float(xu), float(eta_c), float(eta_m), float(prob_m), float(prob_x), float(prob_flip),
                                           int(seed) & 0xFFFFFFFFFFFFFFFF, int(generation), int(row0), int(rows), _fp(out)))
    return out


def ga_duplicates(X, Xoff, device=0):
    """flags int32 [n_off]: offspring row equals a population row or an offspring row below it."""
    lib = _lib()
    X, Xoff = _f32(X), _f32(Xoff)
    flags = np.empty((Xoff.shape[0],), dtype=np.int32)
    _check(lib, lib.glass_op_ga_duplicates(device, X.shape[0], Xoff.shape[0], X.shape[1], _fp(X), _fp(Xoff), flags.ctypes.data_as(ip)))
    return flags


def ga_survive(F, n_pop, pop_out, nsga=True, flags=None, X=None, device=0):
    """Survival over the merged rows F float32 [n_pop + n_off, n_obj] -> dict(chosen, rank, cd, F, counts[, X]); X: merged rows [N, n_var]."""
    lib = _lib()
    F = _f32(F)
    N, M = F.shape
    n_off = N - n_pop
    fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.int32)
    out = dict(chosen=np.empty((pop_out,), np.int32), rank=np.empty((pop_out,), np.int32), cd=np.empty((pop_out,), np.float64),
               F=np.empty((pop_out, M), np.float32), counts=np.empty((2,), np.int32))
    nv, Xp, Xo, Xout = 0, None, None, None
    if X is not None:
        X = _f32(X)
        nv = X.shape[1]
        Xp, Xo = np.ascontiguousarray(X[:n_pop]), np.ascontiguousarray(X[n_pop:])
        Xout = out["X"] = np.empty((pop_out, nv), np.float32)
    _check(lib, lib.glass_op_ga_survive(device, n_pop, n_off, M, pop_out, int(bool(nsga)), _fp(F), None if fl is None else fl.ctypes.data_as(ip),
                                        out["chosen"].ctypes.data_as(ip), out["rank"].ctypes.data_as(ip), out["cd"].ctypes.data_as(dp),
                                        _fp(out["F"]), out["counts"].ctypes.data_as(ip), nv, None if Xp is None else _fp(Xp),
                                        None if Xo is None or not n_off else _fp(Xo), None if Xout is None else _fp(Xout)))
    return out


def ga_migrate(X, F, rank, cd, migrants, nsga=True, device=0):
    """One ring migration (include/glass.h "Device search: islands") of the islands X float32 [K, pop, n_var], F [K, pop, n_obj], rank int32 and
    cd float64 [K, pop] as survival left them -> dict(X, F, rank, cd after it, accepted int32 [K])."""
    lib = _lib()
    X, F = _f32(X), _f32(F)
    K, pop, nv = X.shape
    rank = np.ascontiguousarray(rank, dtype=np.int32)
    cd = np.ascontiguousarray(cd, dtype=np.float64)
    out = dict(X=np.empty_like(X), F=np.empty_like(F), rank=np.empty_like(rank), cd=np.empty_like(cd), accepted=np.empty((K,), np.int32))
    _check(lib, lib.glass_op_ga_migrate(device, K, pop, nv, F.shape[2], int(bool(nsga)), int(migrants), _fp(X), _fp(F), rank.ctypes.data_as(ip),
                                        cd.ctypes.data_as(dp), _fp(out["X"]), _fp(out["F"]), out["rank"].ctypes.data_as(ip),
                                        out["cd"].ctypes.data_as(dp), out["accepted"].ctypes.data_as(ip)))
    return out


# ---- device search: sep-CMA-ES (csrc/cmaes.hip; include/glass.h "Device search: sep-CMA-ES") ---------------------------------------
def cma_sample(mean, diag, sigma, lam, xl, xu, seed=1, generation=0, row0=0, rows=None, X=None, device=0):
    """Rows [row0, row0 + rows) of the generation's lam samples from (mean, diag float64 [n], sigma) -> X float32 [lam, n]; the other rows
    come back as they went in (X: the caller's rows, default NaN)."""
    lib = _lib()
    m = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
    d = np.ascontiguousarray(diag, dtype=np.float64).reshape(-1)
    n = m.size
    rows = lam - row0 if rows is None else rows
    out = np.full((lam, n), np.nan, np.float32) if X is None else _f32(X).copy()
    _check(lib, lib.glass_op_cma_sample(device, int(lam), n, m.ctypes.data_as(dp), d.ctypes.data_as(dp), float(sigma), float(xl), float(xu),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, int(generation), int(row0), int(rows), _fp(out)))
    return out


def cma_rank(F, best_F=np.inf, device=0):
    """F float32 [lam] -> dict(order int32 [lam], finite, updated, best_src, skipped, nonfinite, best_F)."""
    lib = _lib()
    F = _f32(F).reshape(-1)
    order, info, best = np.empty((F.size,), np.int32), np.empty((5,), np.int32), np.empty((1,), np.float32)
    _check(lib, lib.glass_op_cma_rank(device, F.size, _fp(F), float(best_F), order.ctypes.data_as(ip), info.ctypes.data_as(ip), _fp(best)))
    return dict(order=order, finite=int(info[0]), updated=int(info[1]), best_src=int(info[2]), skipped=int(info[3]), nonfinite=int(info[4]),
                best_F=float(best[0]))


def cma_update(X, F, state, xl, xu, generation, device=0):
    """Rank + update of one generation.  X float32 [lam, n], F float32 [lam]; state: dict(m, d, ps, pc float64 [n]; sigma, ps_norm; h, finite,
    updated, skipped, updates; best_X float32 [n], best_F) -> the same dict after the generation, plus order int32 [lam] and best_src."""
    lib = _lib()
    X, F = _f32(X), _f32(F).reshape(-1)
    lam, n = X.shape
    st = np.ascontiguousarray(np.concatenate([np.asarray(state[k], np.float64).reshape(-1) for k in ("m", "d", "ps", "pc")]))
    sd = np.array([state["sigma"], state.get("ps_norm", 0.0)], np.float64)
    si = np.array([state.get(k, 0) for k in ("h", "finite", "updated", "skipped", "updates")] + [-1], np.int32)
    best_X = _f32(state["best_X"]).reshape(-1).copy()
    best_F = np.array([state["best_F"]], np.float32)
    order = np.empty((lam,), np.int32)
    _check(lib, lib.glass_op_cma_update(device, lam, n, _fp(X), _fp(F), st.ctypes.data_as(dp), sd.ctypes.data_as(dp), si.ctypes.data_as(ip),
                                        float(xl), float(xu), int(generation), _fp(best_X), _fp(best_F), order.ctypes.data_as(ip)))
    out = dict(zip(("m", "d", "ps", "pc"), st.reshape(4, n)))
    out.update(sigma=float(sd[0]), ps_norm=float(sd[1]), best_X=best_X, best_F=float(best_F[0]), order=order, best_src=int(si[5]))
    out.update(zip(("h", "finite", "updated", "skipped", "updates"), (int(v) for v in si[:5])))
    return out
