"""The float64 per-operation references the BigGAN kernel tests use (tests/biggan_ops_ref.py), composed the way the engine composes its
kernels (csrc/biggan.cpp: every norm folded into a conv, nearest x2 and the channel-drop skip as addressing, gamma folded into o_conv),
reproduce oracle/biggan_ref.py's gen_block / self_attn / the last three lines of generator on the bg_mini synthetic state.  CPU only.

Bars.  The oracle functions run in float64 when they are fed float64 tensors, so the bar is float64 round-off: 1e-11 * max|ref| (sums of
up to 9 * 256 products of O(1) terms, a few dozen ulp of 2.2e-16).  One oracle function forces float32: latent_forward casts z and the
class bits with .float() (latent.py:16-24 does), so `cond` is compared at 1e-6 * max|ref| (float32 softmax over 24 classes)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import biggan_ops_ref as R
import glass_models as M
from clip_glass_amd import synth
from oracle import biggan_ref

NAME = "bg_mini"
CFG = M.BIGGAN_CONFIGS[NAME]
EPS, NS, G = 1e-4, 51, "biggan.generator."


@pytest.fixture(scope="module")
def state():
    sd = M.make_biggan_state(NAME, 0)
    sd = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items() if k.startswith("biggan.")}
    return sd, {k: torch.from_numpy(v) for k, v in sd.items()}


def sn(sd, prefix):
    """weight_orig / (u . (W_mat v)) in numpy."""
    w = sd[prefix + ".weight_orig"]
    return w / float(sd[prefix + ".weight_u"] @ (w.reshape(w.shape[0], -1) @ sd[prefix + ".weight_v"]))


def _stat(sd, name, truncation):
    return biggan_ref.stat_row(torch.from_numpy(sd[name]), truncation, NS).numpy()


def _tabs(sd, p, cnd, truncation):
    """(A, S) of bn_0 .. bn_3 of block p; S_1 .. S_3 carry the bias of the conv before them."""
    out = []
    for k in range(4):
        b = p + ".bn_%d" % k
        out.append(R.bn_affine(cnd, sn(sd, b + ".scale"), sn(sd, b + ".offset"), _stat(sd, b + ".running_means", truncation),
                               _stat(sd, b + ".running_vars", truncation), EPS,
                               prebias=sd[p + ".conv_%d.bias" % (k - 1)] if k else None))
    return out


def _close(name, got, ref, rel):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    assert err <= rel * float(np.abs(ref).max()), "%s: max err %.3e vs max|ref| %.3e" % (name, err, np.abs(ref).max())


def _blocks():
    """(layer index m in the state dict, up, cin, cout) of every GenBlock."""
    out, m = [], 0
    for i, (up, ci, co) in enumerate(CFG["layers"]):
        if i == CFG["attention_pos"]:
            m += 1
        out.append((m, up, CFG["ch"] * ci, CFG["ch"] * co))
        m += 1
    return out


def _inputs(seed, B, cin, H, W):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, H, W, cin)), rng.standard_normal((B, 2 * CFG["z_dim"]))


@pytest.mark.parametrize("truncation", [1.0, 0.41])
@pytest.mark.parametrize("blk", range(len(CFG["layers"])))
def test_composed_gen_block_matches_the_oracle(state, blk, truncation):
    sd, sdt = state
    m, up, cin, cout = _blocks()[blk]
    p = G + "layers.%d" % m
    x, cnd = _inputs(10 + blk, 2, cin, 4, 6)                 # non-square: an H / W swap in the x2 addressing shows
    w = [sn(sd, p + ".conv_%d" % k) for k in range(4)]
    got, _ = R.gen_block(x, w, sd[p + ".conv_3.bias"], _tabs(sd, p, cnd, truncation), up)
    with torch.no_grad():
        ref = biggan_ref.gen_block(sdt, p, torch.from_numpy(x.transpose(0, 3, 1, 2).copy()), torch.from_numpy(cnd), truncation, cin, cout, up,
                                   NS, EPS)
    _close("gen_block %d" % blk, got.transpose(0, 3, 1, 2), ref.numpy(), 1e-11)


def test_composed_self_attention_matches_the_oracle(state):
    sd, sdt = state
    m = CFG["attention_pos"]
    p = G + "layers.%d" % m
    C = CFG["ch"] * CFG["layers"][m][1]
    x, _ = _inputs(20, 2, C, 6, 8)
    got = R.self_attn(x, *(sn(sd, p + ".snconv1x1_" + k) for k in ("theta", "phi", "g", "o_conv")), sd[p + ".gamma"][0])
    with torch.no_grad():
        ref = biggan_ref.self_attn(sdt, p, torch.from_numpy(x.transpose(0, 3, 1, 2).copy()))
    _close("self_attn", got.transpose(0, 3, 1, 2), ref.numpy(), 1e-11)


def test_composed_tail_matches_the_oracle(state):
    """The last block's first three convs, then `tail` (conv_3 + skip, final bn + relu, conv_to_rgb[:3], tanh) against gen_block + the
    last three lines of biggan_ref.generator; `final` on the oracle's block output likewise (the unfused path's last conv)."""
    sd, sdt = state
    m, up, cin, cout = _blocks()[-1]
    assert up
    p = G + "layers.%d" % m
    x, cnd = _inputs(30, 2, cin, 4, 6)
    w = [sn(sd, p + ".conv_%d" % k) for k in range(4)]
    _, h = R.gen_block(x, w, sd[p + ".conv_3.bias"], _tabs(sd, p, cnd, 1.0), up)
    b = G + "bn"
    inv = 1.0 / np.sqrt(_stat(sd, b + ".running_vars", 1.0) + EPS)
    A = sd[b + ".weight"] * inv
    S = sd[b + ".bias"] - _stat(sd, b + ".running_means", 1.0) * A
    rgb_w, rgb_b = sn(sd, G + "conv_to_rgb"), sd[G + "conv_to_rgb.bias"]
    got = R.tail(h, x, w[3], sd[p + ".conv_3.bias"], A, S, rgb_w, rgb_b)
    with torch.no_grad():
        hb = biggan_ref.gen_block(sdt, p, torch.from_numpy(x.transpose(0, 3, 1, 2).copy()), torch.from_numpy(cnd), 1.0, cin, cout, up, NS, EPS)
        ref = F.relu(biggan_ref.batchnorm(sdt, b, hb, 1.0, None, NS, EPS))
        ref = torch.tanh(biggan_ref.snconv(sdt, G + "conv_to_rgb", ref, padding=1)[:, :3])
    _close("tail", got, ref.numpy(), 1e-11)
    _close("final", R.final(hb.numpy().transpose(0, 2, 3, 1), A, S, rgb_w, rgb_b), ref.numpy(), 1e-11)


def test_cond_matches_the_oracle(state):
    sd, sdt = state
    zd, nc = CFG["z_dim"], CFG["num_classes"]
    x = synth.biggan_population(4, 5, zd, nc)
    x[0, :zd] *= 3.0                                           # beyond the clip
    x[1, zd:] = np.linspace(-50, 50, nc)
    z, probs = biggan_ref.latent_forward(x, zd)                # float32: the function casts with .float()
    ref = torch.cat((z, F.linear(probs, sdt["biggan.embeddings.weight"].float())), dim=1)
    _close("cond", R.cond(x, sd["biggan.embeddings.weight"], zd), ref.numpy(), 1e-6)


def test_table_operands_give_the_same_affine(state):
    """bn_tables (the engine's operands: one dense weight of gain | offset columns, inv_std, mean, prebias) == bn_affine."""
    sd, _ = state
    p = G + "layers.1"
    rng = np.random.default_rng(40)
    cnd = rng.standard_normal((3, 2 * CFG["z_dim"]))
    b = p + ".bn_1"
    Ws, Wo = sn(sd, b + ".scale"), sn(sd, b + ".offset")
    mean, var, pb = _stat(sd, b + ".running_means", 1.0), _stat(sd, b + ".running_vars", 1.0), sd[p + ".conv_0.bias"]
    C = mean.shape[0]
    A, S = R.bn_affine(cnd, Ws, Wo, mean, var, EPS, prebias=pb)
    tab = R.bn_tables(cnd, np.concatenate([Ws.T, Wo.T], axis=1), np.concatenate([np.ones(C), np.zeros(C)]), 1.0 / np.sqrt(var + EPS), mean, pb)
    _close("A", tab[:, :C], A, 1e-13)
    _close("S", tab[:, C:], S, 1e-13)


def test_attn_split_small_example():
    """2 x 4 map, c8 = 1, c2 = 2: the pooled value is the max of the 2 x 2 window, gT is channel-major."""
    T = np.arange(2 * 4 * 4, dtype=np.float64).reshape(1, 2, 4, 4)
    T[0, 0, 1, 1] = 100.0                                      # phi of pixel (0, 1)
    T[0, 1, 2, 3] = -1.0                                       # g channel 1 of pixel (1, 2)
    theta, phi, gT = R.attn_split(T, 1, 2)
    assert theta[0, :, 0].tolist() == [0, 4, 8, 12, 16, 20, 24, 28]
    assert phi[0, :, 0].tolist() == [100.0, 29.0]
    assert gT[0].tolist() == [[22.0, 30.0], [23.0, 31.0]]
