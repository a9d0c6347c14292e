"""float64 numpy references of the GPT-2 trunk's operations, one per kernel family of csrc/gpt2.hip (test infrastructure).

Conventions are the kernels': weights W [N, K] (out = A @ W^T), caches [P, Tmax, D], qkv rows [q | k | v] of D = 64 * heads each.
`forward_cached` composes them into the model (prefill, then single-token steps over the caches); tests/test_gpt2_ops_ref.py pins
that composition to oracle/gpt2_ref.forward, so the GPU tests that use these functions compare against the model and not against a
restatement of the kernels."""
import numpy as np

EPS = 1e-5


def f64(a):
    return np.asarray(a, dtype=np.float64)


def ln_stats(x):
    """Row statistics {mean, rstd} of the TF-style LayerNorm (eps inside the square root)."""
    x = f64(x)
    mean = x.mean(-1)
    var = ((x - mean[..., None]) ** 2).mean(-1)
    return np.stack([mean, 1.0 / np.sqrt(var + EPS)], axis=-1)


def layernorm(x, g, b):
    x = f64(x)
    st = ln_stats(x)
    return (x - st[..., 0:1]) * st[..., 1:2] * f64(g) + f64(b)


def gelu(v):
    v = f64(v)
    return 0.5 * v * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (v + 0.044715 * v ** 3)))


def gemm(a, w, bias=None, mode=0, res=None, ln=None):
    """out = [LN](a) @ w^T (+ bias); mode 1: GELU-tanh; mode 2: res + ."""
    a = f64(a)
    if ln is not None:
        a = layernorm(a, ln[0], ln[1])
    v = a @ f64(w).T
    if bias is not None:
        v = v + f64(bias)
    if mode == 1:
        v = gelu(v)
    elif mode == 2:
        v = v + f64(res)
    return v


def gemm_scale(a, w, bias=None, res=None):
    """The magnitude an element's rounding errors scale with: |a| @ |w|^T + |bias| + |res|."""
    s = np.abs(f64(a)) @ np.abs(f64(w)).T
    if bias is not None:
        s = s + np.abs(f64(bias))
    if res is not None:
        s = s + np.abs(f64(res))
    return s


def attention(qkv, kc, vc, past, heads):
    """qkv [P * nd, 3 D] for positions past .. past + nd - 1; kc / vc [P, Tmax, D].  Appends k / v to copies of the caches, then
    w = q.k / 8, keys j > past + i masked to -1e10, softmax, a = w @ v.  Returns (out [P * nd, D], kc, vc)."""
    kc, vc = np.array(kc, dtype=np.float64), np.array(vc, dtype=np.float64)
    P, _, D = kc.shape
    assert D == 64 * heads
    qkv = f64(qkv).reshape(P, -1, 3 * D)
    nd = qkv.shape[1]
    ns = past + nd
    kc[:, past:ns] = qkv[:, :, D:2 * D]
    vc[:, past:ns] = qkv[:, :, 2 * D:]
    q = qkv[:, :, :D].reshape(P, nd, heads, 64).transpose(0, 2, 1, 3)
    k = kc[:, :ns].reshape(P, ns, heads, 64).transpose(0, 2, 1, 3)
    v = vc[:, :ns].reshape(P, ns, heads, 64).transpose(0, 2, 1, 3)
    s = q @ k.transpose(0, 1, 3, 2) / 8.0
    masked = np.arange(ns)[None, :] > past + np.arange(nd)[:, None]
    s = np.where(masked, -1e10, s)
    s = np.exp(s - s.max(-1, keepdims=True))
    s = s / s.sum(-1, keepdims=True)
    out = (s @ v).transpose(0, 2, 1, 3).reshape(P * nd, D)
    return out, kc, vc


def head(x, wte, g, b):
    """logits = LN_f(x) @ wte^T."""
    return layernorm(x, g, b) @ f64(wte).T


def block_pairs(logits):
    """Stage 1 of the arg-max on given logits [M, V]: per 32-column block the maximum and its lowest index -> ([M, NB], [M, NB])."""
    M, V = logits.shape
    NB = (V + 31) // 32
    pad = np.full((M, NB * 32), -np.inf, dtype=logits.dtype)
    pad[:, :V] = logits
    blk = pad.reshape(M, NB, 32)
    return blk.max(-1), (blk.argmax(-1) + 32 * np.arange(NB)[None, :]).astype(np.int32)     # argmax: the first maximum


def embed(tok, wte, wpe, pos):
    return f64(wte)[np.asarray(tok)] + f64(wpe)[np.asarray(pos)]


def layer_weights(sd, i):
    """Layer i of a `gpt2.transformer.*` state in the kernels' [N, K] convention (the checkpoint's Conv1D weights are [K, N])."""
    q = "gpt2.transformer.h.%d." % i
    t = lambda k: f64(sd[q + k]).T
    return dict(ln1=(sd[q + "ln_1.weight"], sd[q + "ln_1.bias"]), ln2=(sd[q + "ln_2.weight"], sd[q + "ln_2.bias"]),
                w_qkv=t("attn.c_attn.weight"), b_qkv=sd[q + "attn.c_attn.bias"], w_o=t("attn.c_proj.weight"), b_o=sd[q + "attn.c_proj.bias"],
                w_fc=t("mlp.c_fc.weight"), b_fc=sd[q + "mlp.c_fc.bias"], w_pr=t("mlp.c_proj.weight"), b_pr=sd[q + "mlp.c_proj.bias"])


def n_layers(sd):
    i = 0
    while "gpt2.transformer.h.%d.ln_1.weight" % i in sd:
        i += 1
    return i


def forward_cached(sd, tokens, n_prefill, Tmax=None):
    """The model over tokens [P, T] as the engine walks it: one pass over the first n_prefill positions, then one position at a time
    over the KV caches.  Returns logits [P, T, V] (float64)."""
    p = "gpt2.transformer."
    wte, wpe = sd[p + "wte.weight"], sd[p + "wpe.weight"]
    tokens = np.asarray(tokens)
    P, T = tokens.shape
    D = wte.shape[1]
    heads = D // 64
    Tmax = Tmax or T
    layers = [layer_weights(sd, i) for i in range(n_layers(sd))]
    kcs = [np.full((P, Tmax, D), np.nan) for _ in layers]
    vcs = [np.full((P, Tmax, D), np.nan) for _ in layers]
    logits = []
    past = 0
    for nd in [n_prefill] + [1] * (T - n_prefill):
        x = embed(tokens[:, past:past + nd], wte, wpe, np.arange(past, past + nd)[None, :]).reshape(P * nd, D)
        for l, L in enumerate(layers):
            qkv = gemm(x, L["w_qkv"], L["b_qkv"], ln=L["ln1"])
            att, kcs[l], vcs[l] = attention(qkv, kcs[l], vcs[l], past, heads)
            x = gemm(att, L["w_o"], L["b_o"], mode=2, res=x)
            hid = gemm(x, L["w_fc"], L["b_fc"], mode=1, ln=L["ln2"])
            x = gemm(hid, L["w_pr"], L["b_pr"], mode=2, res=x)
        logits.append(head(x, wte, sd[p + "ln_f.weight"], sd[p + "ln_f.bias"]).reshape(P, nd, -1))
        past += nd
    return np.concatenate(logits, axis=1)
