"""The float64 per-kernel references the small-op GPU tests use (tests/small_ops_ref.py) reproduce the oracle on the CPU: oracle/stylegan2_ref.py
(g_mapping, minibatch_std, the style / demodulation algebra of _mod_conv and util.style_tables, D's dense head), oracle/clip_ref.py (token
assembly + ln_pre, the text embedding, ln_final on the EOT row), torch.cosine_similarity, torch.nn.functional.layer_norm and
oracle/fitness_ref.py's F = (-sim, relu(1 - dis)).  CPU only.

Bars.  Oracle functions that run in float64 when fed float64 tensors: 1e-11 * max|ref| (sums of up to 2048 products, a few dozen ulp of
2.2e-16).  clip_ref._ln and stylegan2_ref.minibatch_std cast to float32 (x.float()) and fitness_ref.evaluate is a float32 pipeline:
2e-6 * max|ref| there (a float32 LayerNorm over <= 128 elements, a mean over <= 512 elements, a 64-term dot product: a few ulp of 6e-8).
The float32 twins must lie within 1e-4 * max|ref| of their float64 form: they are what the GPU bars are derived from, and a twin that
computes something else would make a bar meaningless."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glass_models as M
import small_ops_ref as R
from clip_glass_amd import synth
from oracle import clip_ref, fitness_ref, stylegan2_ref as sg
from util import nhwc, style_tables


def _close(name, got, ref, rel):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    assert err <= rel * float(np.abs(ref).max()), "%s: max err %.3e vs max|ref| %.3e" % (name, err, np.abs(ref).max())


def _t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _rng(seed):
    return np.random.default_rng(seed)


def test_mapping_is_g_mapping():
    L, layers, P = 48, 3, 5
    sd = synth.make_state([s for s in synth.stylegan2_g_spec([16, 16], L, layers) if s[0].startswith("G_mapping.")], 3)
    z = synth.latents(4, P, L)
    with torch.no_grad():
        ref = sg.g_mapping({k: _t64(v) for k, v in sd.items()}, _t64(z)).numpy()
    wt = [np.asarray(sd["G_mapping.main.%d.layer.weight" % i], np.float64).T * (0.01 / math.sqrt(L)) for i in range(layers)]
    b = [np.asarray(sd["G_mapping.main.%d.bias" % i], np.float64) * 0.01 for i in range(layers)]
    _close("mapping", R.mapping(z, wt, b), ref, 1e-11)
    _close("mapping float32 twin", R.mapping(z, wt, b, dt=np.float32), ref, 1e-4)
    x = _t64(z)
    _close("pixelnorm", R.pixelnorm(z), (x * torch.rsqrt(torch.mean(x ** 2, dim=-1, keepdim=True) + 1e-8)).numpy(), 1e-12)


@pytest.mark.parametrize("batch_size,group,C", [(4, 4, 12), (8, 4, 32), (8, 2, 12), (8, 8, 16)])
def test_mbstd_is_minibatch_std(batch_size, group, C):
    B = 2 * batch_size
    x = _rng(C + group).standard_normal((B, C, 4, 4))
    with torch.no_grad():
        ref = torch.cat([sg.minibatch_std(_t64(x[i:i + batch_size]).clone(), group) for i in range(0, B, batch_size)]).numpy()
    d, std = R.mbstd(nhwc(x).reshape(B, 16, C), batch_size, group)
    _close("mbstd features", d.reshape(B, 4, 4, C).transpose(0, 3, 1, 2), ref[:, :C], 2e-6)
    _close("mbstd std channel", np.broadcast_to(std[:, None, None], (B, 4, 4)), ref[:, C], 2e-6)
    d32, std32 = R.mbstd(nhwc(x).reshape(B, 16, C), batch_size, group, dt=np.float32)
    _close("mbstd float32 twin", std32, std, 1e-4)


def test_style_path_is_mod_conv_demodulation():
    """dense (style affine) -> style_norm -> dense(in_sq, mode 2) is the demodulation of _mod_conv: d = rsqrt(sum (w coef style)^2 + eps)
    = dscale / smax, and sn * smax = style; and it is util.style_tables, which the engine-level tests use."""
    P, L, cin, cout = 5, 24, 12, 20
    rng = _rng(11)
    lat, dw, db, W = rng.standard_normal((P, L)), rng.standard_normal((cin, L)), 1 + 0.2 * rng.standard_normal(cin), rng.standard_normal((cout, cin, 3, 3))
    lat[2] *= 30.0                                           # a candidate whose styles are large: smax far from 1
    style = R.dense(lat, (dw / math.sqrt(L)).T, db)
    _close("style affine", style, (sg._dense(_t64(lat), _t64(dw)) + _t64(db)).numpy(), 1e-12)
    sn, smax, eps_row = R.style_norm(style, [(0, cin)])
    wsq = (W ** 2).sum(axis=(2, 3)) / (cin * 9)              # [cout, cin]
    dscale = R.dense(sn, wsq.T, in_sq=True, mode=2, eps_row=eps_row[:, 0])
    wm = _t64(W / math.sqrt(cin * 9))[None] * _t64(style).view(P, 1, cin, 1, 1)
    d = torch.rsqrt((wm.reshape(P, cout, -1) ** 2).sum(-1) + 1e-8).numpy()
    _close("sn * smax", sn * smax, style, 1e-12)
    _close("demodulation", dscale / smax, d, 1e-11)
    t_sn, t_smax, t_ds = style_tables(lat, dw, db, W)        # (float32 outputs)
    _close("style_tables sn", sn, t_sn, 2e-7)
    _close("style_tables smax", smax, t_smax, 2e-7)
    _close("style_tables dscale", dscale, t_ds, 2e-7)
    s32, m32, e32 = R.style_norm(style, [(0, cin)], dt=np.float32)
    _close("style_norm float32 twin", s32, sn, 1e-4)
    _close("demodulation float32 twin", R.dense(s32, wsq.T, in_sq=True, mode=2, eps_row=e32[:, 0], dt=np.float32), dscale, 1e-4)


def test_d_head_is_the_discriminators_dense_head():
    P, CL = 5, 8
    rng = _rng(12)
    x = rng.standard_normal((P, CL, 4, 4))                   # the final conv's output, NCHW as the oracle holds it
    W0, B0, W1, B1 = rng.standard_normal((CL, 16 * CL)), 0.2 * rng.standard_normal(CL), rng.standard_normal((1, CL)), 0.2 * rng.standard_normal(1)
    with torch.no_grad():
        h = sg._bias_act(sg._dense(_t64(x).reshape(P, -1), _t64(W0)), _t64(B0))
        ref = sg._bias_act(sg._dense(h, _t64(W1)), _t64(B1), act=False).numpy()[:, 0]
    # the device's operands (csrc/stylegan2.cpp finalize_discriminator): the map NHWC, dense0's columns permuted to (pixel, channel)
    dfin = nhwc(x).reshape(P, 16 * CL)
    w0 = (W0.reshape(CL, CL, 16).transpose(0, 2, 1) / math.sqrt(16 * CL)).reshape(CL, 16 * CL)
    w1 = W1[0] / math.sqrt(CL)
    _close("d_head", R.d_head(dfin, w0, B0, w1, B1), ref, 1e-11)
    _close("d_head float32 twin", R.d_head(dfin, w0, B0, w1, B1, dt=np.float32), ref, 1e-4)


@pytest.mark.parametrize("M_,D", [(5, 64), (3, 100), (2, 1088)])
def test_layernorm_is_torch_layer_norm(M_, D):
    rng = _rng(D)
    x, g, b = 2 * rng.standard_normal((M_, D)) + 0.5, 1 + 0.1 * rng.standard_normal(D), 0.1 * rng.standard_normal(D)
    _close("layernorm", R.layernorm(x, g, b), F.layer_norm(_t64(x), (D,), _t64(g), _t64(b), 1e-5).numpy(), 1e-12)
    _close("layernorm float32 twin", R.layernorm(x, g, b, dt=np.float32), R.layernorm(x, g, b), 1e-4)


def test_embed_lnpre_is_the_visual_towers_token_assembly():
    """clip_ref.encode_image's lines between conv1 and the transformer, with clip_ref._ln (float32)."""
    P, T, D = 3, 5, 128
    rng = _rng(13)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    pe, cls, pos, g, b = f(P, T - 1, D), f(D), f(T, D), 1 + 0.1 * f(D), 0.1 * f(D)
    with torch.no_grad():
        x = torch.cat([torch.from_numpy(cls).view(1, 1, -1).expand(P, 1, D), torch.from_numpy(pe)], dim=1) + torch.from_numpy(pos)
        ref = clip_ref._ln(x, torch.from_numpy(g), torch.from_numpy(b)).numpy()
    _close("embed_lnpre", R.embed_lnpre(pe, cls, pos, g, b), ref, 2e-6)
    _close("embed_lnpre float32 twin", R.embed_lnpre(pe, cls, pos, g, b, dt=np.float32), ref, 2e-6)


def test_embed_text_and_ln_final_are_encode_text_without_layers():
    """A text tower with no transformer block and an identity projection: clip_ref.encode_text is ln_final(token + positional embedding)
    on each text's EOT row (the arg-max token id)."""
    n, ctx, D, V = 3, 7, 100, 50
    rng = _rng(14)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    sd = {"clip.token_embedding.weight": f(V, D), "clip.positional_embedding": f(ctx, D), "clip.ln_final.weight": 1 + 0.1 * f(D),
          "clip.ln_final.bias": 0.1 * f(D), "clip.text_projection": np.eye(D, dtype=np.float32)}
    tokens = rng.integers(1, V - 1, (n, ctx))
    tokens[0, 0], tokens[1, 3], tokens[2, ctx - 1] = 0, 0, 0
    eot = [2, 6, 4]
    tokens[np.arange(n), eot] = V - 1
    with torch.no_grad():
        ref = clip_ref.encode_text({k: torch.from_numpy(v) for k, v in sd.items()}, torch.from_numpy(tokens), heads=1).numpy()
    x = R.embed_text(tokens, sd["clip.token_embedding.weight"], sd["clip.positional_embedding"])
    np.testing.assert_array_equal(x.astype(np.float32).reshape(n, ctx, D),
                                  sd["clip.token_embedding.weight"][tokens] + sd["clip.positional_embedding"])      # one float32 add: exact in float64
    rows = np.arange(n) * ctx + np.array(eot)
    _close("ln_final on the EOT rows", R.layernorm(x[rows], sd["clip.ln_final.weight"], sd["clip.ln_final.bias"]), ref, 2e-6)


def test_cosine_is_torch_cosine_similarity():
    rng = _rng(15)
    feat, target = rng.standard_normal((5, 100)), rng.standard_normal(100)
    feat[3] = 0.0
    ref = F.cosine_similarity(_t64(feat), _t64(target).view(1, -1), dim=1, eps=1e-8).numpy()
    _close("cosine", R.cosine(feat, target), ref, 1e-12)
    assert R.cosine(feat, target)[3] == 0.0 and R.cosine(feat, target, dt=np.float32)[3] == 0.0
    _close("cosine float32 twin", R.cosine(feat, target, dt=np.float32), ref, 1e-4)
    vs, mean = R.cosine_views(feat.reshape(1, 5, 100), target)
    _close("cosine views", vs[0], ref, 1e-12)
    _close("cosine views mean", mean, [ref.mean()], 1e-12)


def test_assemble_F_and_cosine_are_fitness_refs_objectives():
    """fitness_ref.evaluate on the `mini` networks: F = column_stack(-cosine(features, target), relu(1 - dis)) from the features and logits it
    reports in `detail`."""
    name, P, bs = "mini", 4, 4
    c = M.CONFIGS[name]
    tsd = {k: torch.as_tensor(v) for k, v in M.make_state(name, 0).items()}
    x = synth.latents(1, P, c["latent"])
    target = synth.normal(3, "target", (c["clip"][5],))
    detail = {}
    Fo, _ = fitness_ref.evaluate(tsd, x, target, bs, True, None, clip_size=c["clip"][4], detail=detail)
    dis = detail["dis"].numpy()[:, 0]
    assert (dis < 1).any()                                   # (the hinge is active somewhere)
    got = R.assemble_F(R.cosine(detail["features"].numpy(), target), dis)
    _close("F", got, Fo, 2e-6)
    _close("F, one objective", R.assemble_F(R.cosine(detail["features"].numpy(), target)), Fo[:, :1], 2e-6)
    np.testing.assert_array_equal(R.assemble_F([0.25, -0.5], [0.5, 1.5]), [[-0.25, 0.5], [0.5, 0.0]])


def test_finalize_image_and_image_patches():
    y = np.array([-3.0, -1.0, -0.5, 0.0, 0.25, 1.0, 1.5])
    np.testing.assert_array_equal(R.finalize_image(y), ((torch.from_numpy(y) + 1) / 2.0).clip(0, 1).numpy())      # utils.py:14-17 as fitness_ref.generate
    n, S, ps, D = 2, 28, 14, 6
    rng = _rng(16)
    img, w = rng.standard_normal((n, 3, S, S)), rng.standard_normal((D, 3, ps, ps))
    with torch.no_grad():                                    # clip_ref.encode_image: conv1 with stride = patch, then [n, D, G G] -> [n, G G, D]
        ref = F.conv2d(_t64(img), _t64(w), stride=ps).reshape(n, D, -1).permute(0, 2, 1).reshape(-1, D).numpy()
    _close("patch operand @ conv1.weight.reshape(width, -1)^T", R.image_patches(img, ps) @ w.reshape(D, -1).T, ref, 1e-11)
