"""float64 restatement of CLIP's ModifiedResNet image tower (clip/model.py:9-149) from a state dict, and float64 references for the single
ops the engine builds it from (TEST INFRASTRUCTURE; pinned to the reference's own module by tests/test_clip_resnet_ref.py).

    forward(sd, img)                 the tower: stem, bottlenecks, attention pool -> features [B, embed]
    forward(sd, img, round16=True)   the same with every activation the engine STORES rounded to fp16 (what fp16 storage alone costs)
    bn_affine / conv_bn / avgpool2 / attnpool_tokens    the single ops, NHWC like the diagnostic ops

Also the inputs the tower tests share: TOWER_CASES, tower_state (synthetic weights) and tower_images (low-frequency pattern + noise: rows
that differ by far more than the feature bar, activations that stay small enough for fp16 storage).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from clip_glass_amd import synth

EPS = 1e-5
# name -> (layers, width, res, embed, P): the tower cases of tests/test_gpu_clip_resnet.py
TOWER_CASES = {
    "mini64": ((1, 1, 1, 1), 64, 64, 64, 3),
    "mini96": ((1, 1, 1, 1), 64, 96, 64, 3),          # maps 24 / 12 / 6 / 3, 10 tokens
    "nodown64": ((2, 1, 1, 2), 64, 64, 128, 2),       # second blocks of stages 1 and 4: no downsample branch
    "rn50": ((3, 4, 6, 3), 64, 224, 1024, 4),
}
PIN_CASES = ("mini64", "mini96", "nodown64")          # tests/golden/clip_resnet_pins.npz (a few KB)
FEATURE_BAR = 5e-3


def h16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def tower_state(case, seed=11):
    layers, width, res, embed, _ = TOWER_CASES[case]
    return synth.make_state(synth.clip_resnet_spec(layers, width, res, embed), seed)


def tower_images(case, seed=12):
    """[P,3,res,res] float32, already fp16 values: 0.5 * white noise + 1.5 * (a random 4 x 4 pattern per image and channel, bilinearly
    upsampled).  White noise alone averages out in the tower: two such images gave feature rows with cosine 0.9996."""
    _, _, res, _, P = TOWER_CASES[case]
    noise = synth.normal(seed, "rn_noise_" + case, (P, 3, res, res))
    pat = torch.tensor(synth.normal(seed, "rn_pattern_" + case, (P, 3, 4, 4)))
    up = F.interpolate(pat, size=(res, res), mode="bilinear", align_corners=False).numpy()
    return h16(0.5 * noise + 1.5 * up)


# ---- single ops (NHWC, float64) ------------------------------------------------------------------------------------------------------
def bn_affine(sd, prefix):
    """Inference BatchNorm as scale and shift: A = gamma / sqrt(var + eps), S = beta - mean * A."""
    g, b, mu, var = (np.asarray(sd[prefix + k], np.float64) for k in (".weight", ".bias", ".running_mean", ".running_var"))
    a = g / np.sqrt(var + EPS)
    return a, b - mu * a


def conv_bn(x, w, a, s, stride=1, res=None, relu=True):
    """act(conv(x, w, pad = ks // 2) * a + s (+ res)) with the residual added BEFORE the ReLU; x, res NHWC, w [Cout,Cin,ks,ks]."""
    xt = torch.as_tensor(np.asarray(x, np.float64)).permute(0, 3, 1, 2)
    wt = torch.as_tensor(np.asarray(w, np.float64))
    y = F.conv2d(xt, wt, stride=stride, padding=wt.shape[-1] // 2).permute(0, 2, 3, 1).numpy()
    y = y * np.asarray(a, np.float64) + np.asarray(s, np.float64)
    if res is not None:
        y = y + np.asarray(res, np.float64)
    return np.maximum(y, 0) if relu else y


def avgpool2(x):
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    return x.reshape(B, H // 2, 2, W // 2, 2, C).mean(axis=(2, 4))


def attnpool_tokens(x, pos):
    """x [B,HW,C] -> [B,HW+1,C] = [mean over HW ; the HW pixels] + pos (clip/model.py:66-68)."""
    x = np.asarray(x, np.float64)
    return np.concatenate([x.mean(axis=1, keepdims=True), x], axis=1) + np.asarray(pos, np.float64)[None]


# ---- the tower -----------------------------------------------------------------------------------------------------------------------
def _stages(sd, v):
    return [len(set(k.split(".")[3] for k in sd if k.startswith("%slayer%d." % (v, b)))) for b in (1, 2, 3, 4)]


def forward(sd, img, round16=False, prefix="clip.visual."):
    """ModifiedResNet.forward on img [B,3,S,S] -> float64 [B, embed].  round16: the maps, tokens, q|k|v and attention rows the engine stores
    as fp16 are rounded to fp16 where it stores them (conv weights are fp16 values in either mode, as a converted checkpoint's are)."""
    v = prefix
    r = (lambda t: h16(t).astype(np.float64)) if round16 else (lambda t: t)
    W = lambda k: h16(sd[v + k + ".weight"]).astype(np.float64)
    x = np.asarray(img, np.float64).transpose(0, 2, 3, 1)
    for i, stride in ((1, 2), (2, 1), (3, 1)):
        x = r(conv_bn(x, W("conv%d" % i), *bn_affine(sd, v + "bn%d" % i), stride=stride))
    x = r(avgpool2(x))
    for st, n in enumerate(_stages(sd, v)):
        for i in range(n):
            p = "layer%d.%d." % (st + 1, i)
            stride = 2 if (st > 0 and i == 0) else 1
            out = r(conv_bn(x, W(p + "conv1"), *bn_affine(sd, v + p + "bn1")))
            out = r(conv_bn(out, W(p + "conv2"), *bn_affine(sd, v + p + "bn2")))
            if stride > 1:
                out = r(avgpool2(out))
            identity = x
            if v + p + "downsample.0.weight" in sd:
                xd = r(avgpool2(x)) if stride > 1 else x
                identity = r(conv_bn(xd, W(p + "downsample.0"), *bn_affine(sd, v + p + "downsample.1"), relu=False))
            x = r(conv_bn(out, W(p + "conv3"), *bn_affine(sd, v + p + "bn3"), res=identity, relu=True))
    B, H, _, C = x.shape
    a = v + "attnpool."
    tok = r(attnpool_tokens(x.reshape(B, H * H, C), sd[a + "positional_embedding"]))
    heads = C // 64
    qkv = []
    for name in ("q_proj", "k_proj", "v_proj"):
        t = tok @ h16(sd[a + name + ".weight"]).astype(np.float64).T + np.asarray(sd[a + name + ".bias"], np.float64)
        qkv.append(r(t).reshape(B, H * H + 1, heads, 64).transpose(0, 2, 1, 3))
    q, k, val = qkv
    att = (q * 0.125) @ k.transpose(0, 1, 3, 2)
    att = np.exp(att - att.max(axis=-1, keepdims=True))
    att = att / att.sum(axis=-1, keepdims=True)
    o = r((att @ val).transpose(0, 2, 1, 3).reshape(B, H * H + 1, C))
    # only token 0 leaves the pool; c_proj stays fp32 in the engine
    return o[:, 0] @ np.asarray(sd[a + "c_proj.weight"], np.float64).T + np.asarray(sd[a + "c_proj.bias"], np.float64)


@functools.lru_cache(maxsize=None)
def tower_reference(case, round16=False):
    """Features of a tower case, computed once per process and shared by the tests that need them (do not modify the array)."""
    out = forward(tower_state(case), tower_images(case), round16=round16)
    out.setflags(write=False)
    return out
