"""GPT-2 stochastic decode (config GPT2 with stochastic=True; reference gpt2/sample.py:10-36 with sample=True, models.py:45-60).

torch.multinomial's random stream cannot be reproduced, so parity is defined against one rule (csrc/gpt2.hip, gpt2_sample_kernel):
l' = l / T in fp32, keep l' >= the k-th largest l' (ties included), p ~ exp(l' - max l'), u from Philox at (row, step, generation,
purpose) (synth.gpt2_sample_uniform), token = the first kept index whose running sum of p exceeds u * sum(p).  The rule's
probabilities are pinned to the reference's top_k_logits + softmax; the device is checked against a float64 mirror of the rule."""
import types

import numpy as np
import pytest
import torch

from clip_glass_amd import synth
from oracle import gpt2_ref
from util import diag

MINI = dict(n_embd=128, n_layer=2, vocab=2048)
MID = dict(n_embd=256, n_layer=3, vocab=5000)
WIDE = dict(n_embd=256, n_layer=3, vocab=8192)


# ---- the rule, float64 ---------------------------------------------------------------------------------------------------------------
def _scaled(logits, T):
    """l' as the device computes it: an fp32 division by the fp32 temperature."""
    return (np.asarray(logits, np.float32) / np.float32(T)).astype(np.float64)


def _kept(lp, k):
    V = lp.shape[-1]
    if k == 0 or k >= V:
        return np.ones(lp.shape, bool)
    m = -np.sort(-lp, axis=-1)[..., k - 1:k]
    return lp >= m


def _weights(lp, k):
    """Unnormalised p over the kept set (1 where l' equals the row maximum; 0 outside the kept set)."""
    mx = lp.max(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.where(lp == mx, 1.0, np.exp(lp - mx))
    return np.where(_kept(lp, k), e, 0.0)


def _probs(lp, k):
    w = _weights(np.asarray(lp, np.float64), k)
    return w / w.sum(axis=-1, keepdims=True)


def _mirror_pick(lp_row, k, u):
    """(token, CDF margin / sum p, k-th threshold gap) of one row under the rule."""
    w = _weights(lp_row[None], k)[0]
    kept = _kept(lp_row[None], k)[0]
    cum = np.cumsum(w)
    target = u * cum[-1]
    hit = np.nonzero(kept & (cum > target))[0]
    tok = int(hit[0]) if hit.size else int(np.nonzero(kept)[0][-1])
    margin = float(np.min(np.abs(cum[kept] - target)) / cum[-1])
    V = lp_row.shape[0]
    gap = np.inf
    if 0 < k < V:
        s = -np.sort(-lp_row)
        with np.errstate(invalid="ignore"):
            gap = float(s[k - 1] - s[k])            # (nan for two -inf values: no near-threshold escape)
    return tok, margin, gap


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.reference
def test_probability_rule_matches_reference_top_k_softmax():
    """_probs(l / 0.7, 40) == softmax(top_k_logits(l / 0.7, 40)) of the reference's own gpt2/sample.py, random rows and a tie at the
    40th value (both tied entries kept, as torch.where(l < m) keeps them)."""
    import ref_harness as rh
    if not rh.available():
        pytest.skip("/root/reference not present")
    sd = synth.make_state(synth.gpt2_spec(**MINI, n_positions=64), 2)
    _, sample_sequence = rh.build_ref_gpt2(sd, MINI["n_embd"], MINI["n_layer"], MINI["vocab"])
    top_k_logits = sample_sequence.__globals__["top_k_logits"]
    rs = np.random.RandomState(0)
    l = rs.randn(6, 3000) * 3.0
    srt = -np.sort(-l[5])
    l[5, np.argsort(-l[5])[45]] = srt[39]                   # row 5: a tie at the 40th value
    for k in (40, 0, 1):
        lt = torch.tensor(l, dtype=torch.float64) / 0.7
        ref = torch.softmax(top_k_logits(lt, k), dim=-1).numpy()
        got = _probs(l / 0.7, k)
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-7)
    assert (_probs(l[5:6] / 0.7, 40) > 0).sum() == 41


def test_sample_uniform_stream():
    """synth.gpt2_sample_uniform: values in (0, 1), distinct across row / step / generation / purpose, and not the noise planes' words
    for the same counters (the tag in the key)."""
    rows, steps, gens = np.meshgrid(np.arange(64), np.arange(31), np.arange(4), indexing="ij")
    u = synth.gpt2_sample_uniform(7, gens, rows, steps)
    assert u.dtype == np.float64 and (u > 0).all() and (u < 1).all()
    assert np.unique(u).size == u.size
    u_save = synth.gpt2_sample_uniform(7, gens, rows, steps, synth.GPT2_SAMPLE_SAVE)
    assert not np.isin(u_save, u).any()
    raw = synth.philox4x32(rows, steps, gens.astype(np.uint32), 0, 7, 0)[0]
    x = np.round(u * 2.0 ** 32 - 0.5).astype(np.uint64)
    assert not (x == raw.astype(np.uint64)).any()
    assert synth.gpt2_sample_uniform(7, 0, 3, 5) != synth.gpt2_sample_uniform(8, 0, 3, 5)


class _StubEngine:
    def __init__(self):
        self.calls = []

    def gpt2_decode(self, ctx, length):
        self.calls.append(("decode", ctx.copy(), length, {}))
        return np.concatenate([ctx, np.zeros((ctx.shape[0], length), ctx.dtype)], axis=1)

    def gpt2_sample(self, ctx, length, **kw):
        self.calls.append(("sample", ctx.copy(), length, kw))
        return np.concatenate([ctx, np.ones((ctx.shape[0], length), ctx.dtype)], axis=1)


def _host_gpt2(**over):
    from clip_glass_amd import config as gconfig
    from clip_glass_amd.models import GPT2
    cfg = types.SimpleNamespace(config="GPT2")
    vars(cfg).update(gconfig.get_config("GPT2"))
    vars(cfg).update(weights="synthetic:0", encoder_size=64, gpt2_geometry=dict(n_embd=64, n_layer=1), encoder=None, vocab=None)
    vars(cfg).update(over)
    m = GPT2(cfg)
    m.engine = _StubEngine()
    m.enc = types.SimpleNamespace(eot=63, decode=lambda toks: " ".join(map(str, toks)))
    return m


def test_host_plumbing_stochastic_and_greedy():
    """GPT2.generate: stochastic -> gpt2_sample(T 0.7, k 40, the configured seed, the generation, first_row 0); greedy ->
    gpt2_decode as before; Generator's purpose words; run.py --stochastic."""
    z = np.arange(40).reshape(2, 20) % 60
    m = _host_gpt2(stochastic=True, seed=5)
    texts = m.generate(z, generation=3)
    assert len(texts) == 2
    kind, ctx, length, kw = m.engine.calls[-1]
    assert kind == "sample" and length == 30 and ctx.shape == (2, 23)
    assert kw == dict(temperature=0.7, top_k=40, seed=5, generation=3, first_row=0, purpose=synth.GPT2_SAMPLE_EVALUATE)
    m.generate(z, generation=4, purpose=synth.GPT2_SAMPLE_SAVE)
    assert m.engine.calls[-1][3]["purpose"] == synth.GPT2_SAMPLE_SAVE != synth.GPT2_SAMPLE_EVALUATE
    m = _host_gpt2(stochastic=True, sample_seed=11, seed=5, temperature=1.3, top_k=7)
    m.generate(z)
    assert m.engine.calls[-1][3] == dict(temperature=1.3, top_k=7, seed=11, generation=0, first_row=0, purpose=0)
    m = _host_gpt2(stochastic=True)
    m.generate(z)
    assert m.engine.calls[-1][3]["seed"] == 0
    m = _host_gpt2()                                       # the table's stochastic=False
    m.generate(z, generation=9)
    kind, ctx, length, kw = m.engine.calls[-1]
    assert kind == "decode" and length == 30 and kw == {}
    np.testing.assert_array_equal(ctx[:, 20:], np.tile(m.init_tokens, (2, 1)))
    from clip_glass_amd import run
    assert run.build_parser().parse_args(["--stochastic"]).stochastic is True
    assert not run.build_parser().parse_args([]).stochastic


# ---- GPU: the op against the mirror ---------------------------------------------------------------------------------------------------
def _crafted_rows(V, k, seed):
    rs = np.random.RandomState(seed)
    l = (rs.randn(12, V) * 3.0).astype(np.float32)
    kk = min(max(k, 1), V)
    for r in (1, 2):                                       # ties at the k-th value
        order = np.argsort(-l[r], kind="stable")
        v = l[r, order[kk - 1]]
        l[r, order[kk:kk + 3 * r]] = v
    l[3, rs.choice(V, V // 3, replace=False)] = -1e10      # masked entries
    l[4, rs.choice(V, V // 3, replace=False)] = -np.inf
    l[5] = 1.5                                             # one value everywhere: every block is a candidate
    l[6] = -np.inf
    l[6, rs.choice(V, min(3, V), replace=False)] = 0.25    # a few finite entries in an -inf row
    l[7, :] = np.round(l[7] * 2) / 2                        # coarse values: ties all over the row
    l[8, V // 2] = 40.0                                    # one dominant entry
    return l


@pytest.mark.gpu
@pytest.mark.parametrize("V", [50257, 5000, 2048, 33])
@pytest.mark.parametrize("k", [0, 1, 40, 256])
def test_op_sample_matches_mirror(V, k):
    from clip_glass_amd import ops
    T, seed, gen, row0, step = 0.7, 1234567890123, 5, 100, 3
    l = _crafted_rows(V, k, V + k)
    got = ops.gpt2_sample(l, T, k, seed, gen, row0, step)
    u = synth.gpt2_sample_uniform(seed, gen, row0 + np.arange(l.shape[0]), step)
    lp = _scaled(l, T)
    kept = _kept(lp, k)
    near = 0
    for r in range(l.shape[0]):
        assert kept[r, got[r]], "V=%d k=%d row %d: token %d outside the kept set" % (V, k, r, got[r])
        tok, margin, _ = _mirror_pick(lp[r], k, u[r])
        if got[r] != tok:
            diag("[gpt2-sample] op V=%d k=%d row %d NEAR-BOUNDARY EXCEPTION: device %d mirror %d, CDF margin %.3e" % (V, k, r, got[r], tok, margin))
            assert margin < 1e-5, "V=%d k=%d row %d: device %d, mirror %d, margin %.3e" % (V, k, r, got[r], tok, margin)
            near += 1
    assert near <= 1
    # purpose and step select other draws; the same arguments the same draw
    np.testing.assert_array_equal(ops.gpt2_sample(l, T, k, seed, gen, row0, step), got)


@pytest.mark.gpu
def test_op_sample_rejects_unsupported_arguments():
    from clip_glass_amd import ops
    l = np.zeros((2, 64), np.float32)
    for T, k in ((0.0, 40), (-1.0, 40), (float("inf"), 40), (0.7, -1), (0.7, 257)):
        with pytest.raises(RuntimeError):
            ops.gpt2_sample(l, T, k, 0, 0, 0, 0)


@pytest.mark.gpu
def test_op_sample_distribution_chi_square():
    """One crafted row over 8192 global rows (fixed seeds: deterministic): the token histogram fits the rule's probabilities."""
    from scipy.stats import chi2
    from clip_glass_amd import ops
    V, k, T, n = 5000, 40, 0.7, 8192
    rs = np.random.RandomState(3)
    row = (rs.randn(V) * 1.0).astype(np.float32)
    row[rs.choice(V, 45, replace=False)] = np.linspace(0.5, 3.0, 45).astype(np.float32)
    row[rs.choice(V, 4, replace=False)] = -np.inf
    logits = np.tile(row, (n, 1))
    got = ops.gpt2_sample(logits, T, k, 99, 2, 0, 1)
    p = _probs(_scaled(row[None], T), k)[0]
    assert p[got].min() > 0
    exp = p * n
    big = exp >= 5
    obs = np.bincount(got, minlength=V).astype(np.float64)
    o = np.append(obs[big], obs[~big].sum())
    e = np.append(exp[big], exp[~big].sum())
    if e[-1] == 0:
        o, e = o[:-1], e[:-1]
    stat = float(((o - e) ** 2 / e).sum())
    pval = float(chi2.sf(stat, len(o) - 1))
    diag("[gpt2-sample] chi-square over %d rows: %d bins, stat %.1f, p %.3g" % (n, len(o), stat, pval))
    assert pval > 1e-4


# ---- GPU: the engine ------------------------------------------------------------------------------------------------------------------
def _engine(geo, P, seed=2):
    import glass_models as M
    from clip_glass_amd.engine import Engine
    sd = synth.make_state(synth.gpt2_spec(**geo, n_positions=64), seed)
    clip = M.CONFIGS["mini"]["clip"]
    sd.update(synth.make_state(synth.clip_visual_spec(clip[0], clip[1], clip[3], clip[4], clip[5]), 0))
    e = Engine([], latent_size=4, mapping_layers=0, batch_size=1, use_discriminator=False, n_obj=1, max_pop=P, clip=clip, noise_mode=0)
    e.load_state(sd)
    e.finalize()
    return e, sd


def _ctx(seed, P, n, vocab):
    return np.random.RandomState(seed).randint(0, vocab, size=(P, n)).astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("geo", [MINI, MID, WIDE], ids=["mini-generic", "v5000-fused", "v8192-fused"])
def test_engine_sample_matches_oracle_teacher_forced(geo):
    """At every step the oracle's logits on the device's own prefix plus the mirrored u give the device's token.  Exceptions (logged):
    a CDF margin below 2e-4 or a k-th threshold gap below 1e-4 — the oracle's fp32 logits differ from the device's by summation order
    (the greedy parity test's 1e-4 logit bar)."""
    P, n_ctx, length, T, k, seed, gen, row0 = 16, 23, 10, 0.7, 40, 77, 3, 5
    e, sd = _engine(geo, P)
    ctx = _ctx(1, P, n_ctx, geo["vocab"])
    got = e.gpt2_sample(ctx, length, temperature=T, top_k=k, seed=seed, generation=gen, first_row=row0)
    e.close()
    assert got.shape == (P, n_ctx + length) and np.array_equal(got[:, :n_ctx], ctx)
    tsd = {kk: torch.as_tensor(v) for kk, v in sd.items()}
    exc = 0
    for s in range(length):
        with torch.no_grad():
            lg, _ = gpt2_ref.forward(tsd, torch.tensor(got[:, :n_ctx + s]))
        lp = _scaled(lg[:, -1].numpy(), T)
        u = synth.gpt2_sample_uniform(seed, gen, row0 + np.arange(P), s)
        for r in range(P):
            tok, margin, gap = _mirror_pick(lp[r], k, u[r])
            if got[r, n_ctx + s] != tok:
                diag("[gpt2-sample] %s NEAR-BOUNDARY EXCEPTION: row %d step %d device %d mirror %d, CDF margin %.3e, k-th gap %.3e"
                     % (geo, r, s, got[r, n_ctx + s], tok, margin, gap * T))
                assert margin < 2e-4 or gap * T < 1e-4, "row %d step %d: clear margin %.3e / gap %.3e" % (r, s, margin, gap * T)
                exc += 1
    diag("[gpt2-sample] %s: %d steps x %d rows teacher-forced, %d near-boundary exception(s)" % (geo, length, P, exc))
    assert exc <= 2


@pytest.mark.gpu
@pytest.mark.parametrize("geo", [MINI, MID], ids=["mini-generic", "v5000-fused"])
def test_engine_top_k_1_equals_greedy(geo):
    e, _ = _engine(geo, 16)
    ctx = _ctx(2, 16, 23, geo["vocab"])
    greedy = e.gpt2_decode(ctx, 12)
    samp = e.gpt2_sample(ctx, 12, temperature=0.7, top_k=1, seed=5, generation=1)
    e.close()
    np.testing.assert_array_equal(samp, greedy)


@pytest.mark.gpu
def test_engine_sample_rows_do_not_depend_on_the_launch():
    e, _ = _engine(MID, 72)
    ctx = _ctx(4, 72, 23, MID["vocab"])
    kw = dict(temperature=0.7, top_k=40, seed=123, generation=2)
    whole = e.gpt2_sample(ctx, 12, **kw)
    assert whole.shape == (72, 35)
    for lo, hi in ((0, 8), (8, 72), (0, 64), (64, 72), (3, 5)):
        np.testing.assert_array_equal(e.gpt2_sample(ctx[lo:hi], 12, first_row=lo, **kw), whole[lo:hi])
    np.testing.assert_array_equal(e.gpt2_sample(ctx, 12, **kw), whole)
    other = e.gpt2_sample(ctx, 12, **dict(kw, generation=3))
    save = e.gpt2_sample(ctx, 12, purpose=synth.GPT2_SAMPLE_SAVE, **kw)
    e.close()
    assert (other != whole).any(axis=1).any() and (save != whole).any(axis=1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("geo", [MINI, MID], ids=["mini-generic", "v5000-fused"])
def test_engine_mode_switching_keeps_graphs_apart(geo):
    """greedy -> sample -> greedy -> sample on one engine with one geometry: each equals a fresh engine's result."""
    ctx = _ctx(6, 16, 23, geo["vocab"])
    kw = dict(temperature=0.7, top_k=40, seed=9, generation=1)

    def fresh(fn):
        e, _ = _engine(geo, 16)
        out = fn(e)
        e.close()
        return out
    g_ref = fresh(lambda e: e.gpt2_decode(ctx, 10))
    s_ref = fresh(lambda e: e.gpt2_sample(ctx, 10, **kw))
    assert (g_ref != s_ref).any()
    e, _ = _engine(geo, 16)
    for i in range(2):
        np.testing.assert_array_equal(e.gpt2_decode(ctx, 10), g_ref, err_msg="greedy, round %d" % i)
        np.testing.assert_array_equal(e.gpt2_sample(ctx, 10, **kw), s_ref, err_msg="sample, round %d" % i)
    e.close()


@pytest.mark.gpu
def test_img2txt_stochastic_generation_problem(tmp_path):
    """GPT2 config with stochastic=True through GenerationProblem: finite F [P, 1], fresh texts per generation, and a second problem
    with the same seed repeats the F sequence."""
    import glass_models as M
    from clip_glass_amd import config as gconfig
    from clip_glass_amd.problem import GenerationProblem
    from test_gpt2 import _synthetic_vocabs
    enc, voc, bpe, gvocab, cvocab = _synthetic_vocabs(str(tmp_path))
    clipg = M.CONFIGS["mini"]["clip"]

    def problem():
        cfg = types.SimpleNamespace(config="GPT2", device="cuda", target="unused", seed=4)
        vars(cfg).update(gconfig.get_config("GPT2"))
        vars(cfg).update(weights="synthetic:2", clip_weights="synthetic:0", clip_geometry=clipg,
                         clip_text_geometry=dict(width=64, layers=2, vocab=cvocab), encoder_size=gvocab,
                         gpt2_geometry=dict(n_embd=128, n_layer=2), encoder=enc, vocab=voc, bpe_path=bpe,
                         target_features=synth.normal(3, "imgfeat", (clipg[5],)), pop_size=8, max_pop=8, stochastic=True,
                         init_text="the an")
        return GenerationProblem(cfg), cfg

    x = np.random.RandomState(0).randint(0, gvocab, size=(8, 20))
    runs = []
    for _ in range(2):
        prob, cfg = problem()
        ls = cfg.latent(cfg)
        ls.set_from_population(x)
        Fs, texts = [], []
        for g in range(2):
            F = prob.generator.evaluate(ls)
            assert F.shape == (8, 1) and np.isfinite(F).all()
            Fs.append(F)
            texts.append(list(prob.generator.last_texts))
        saved = prob.generator.generate(ls)
        assert prob.generator.generate(ls) == saved
        prob.generator.engine.close()
        assert texts[0] != texts[1], "two generations drew the same texts"
        runs.append((Fs, texts))
    diag("[gpt2-sample] img2txt stochastic texts: %r / %r" % (runs[0][1][0][:2], runs[0][1][1][:2]))
    for a, b in zip(runs[0][0], runs[1][0]):
        np.testing.assert_array_equal(a, b)
    assert runs[0][1] == runs[1][1]
